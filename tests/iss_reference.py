"""wm_iss_keypoints (libwave_amd/csrc/wm_iss.hip; the rule is in include/wavematch.h, "keypoints") restated in Python:
the checker of tests/test_iss_gpu.py, in the manner of outlier_reference.py and cluster_reference.py.

  neighbours  r2 = (float32) (radius * radius), the product in double; j is a neighbour of finite i iff d2 < r2
              (strict), i itself included; d2 = (dx * dx + dy * dy) + dz * dz in float32, every operation rounded.
  scatter     d = p_j - p_i in float32, widened; the six products in float64 (exact); each enters its sum as the integer
              rint(product * 2^(36 - x)), r2s = m 2^x with m in [0.5, 1); the integers are added exactly.
  saliency    third_from_sums: Python-float restatement of wm_iss_rule.hpp, jacobi3 (wm_math.hpp) included, operation
              by operation -- IEEE double on both sides, so wm_iss_third must equal it bit for bit.
  suppression keypoint iff third > 0, neighbours within r2n >= min_neighbors, no such neighbour with a larger third.
  two forms   keypoints_brute: every pair, Python integers for the sums.  keypoints: candidate pairs from a float64
              kd-tree at radius * 1.001 + 1e-6, the float32 test re-formed on them, int64 numpy sums.
              tests/test_iss_reference_cpu.py holds the two to each other on every case the device is compared on.
  pcl_literal PCL's own arithmetic in float64: double sums in list order, numpy.linalg.eigvalsh, PCL's tests.  The
              CPU test holds its salient and keypoint sets to the rule's, up to points whose own decision lies within
              1e-6 relative of its bound (compare_with_literal)."""
import math

import numpy as np

NONE, PLAIN, SALIENT, KEYPOINT = 0, 1, 2, 3
SCALE_BITS = 36
F = np.float32


def r2_of(radius):
    return F(float(radius) * float(radius))


def exponent_of(r2s):
    """x with r2s = m 2^x, m in [0.5, 1)"""
    return math.frexp(float(r2s))[1]


# ---- the saliency step (wm_iss_rule.hpp, wm_math.hpp jacobi3), Python floats

def _rotate(A, V, P, Q):
    R = 3 - P - Q
    apq = A[P * 3 + Q]
    if apq == 0.0:
        return
    app, aqq = A[P * 3 + P], A[Q * 3 + Q]
    if abs(apq) <= 8.673617379884035e-19 * (abs(app) + abs(aqq)):
        A[P * 3 + Q] = A[Q * 3 + P] = 0.0
        return
    theta = (aqq - app) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    A[P * 3 + P] = app - t * apq
    A[Q * 3 + Q] = aqq + t * apq
    A[P * 3 + Q] = A[Q * 3 + P] = 0.0
    arp, arq = A[R * 3 + P], A[R * 3 + Q]
    A[R * 3 + P] = A[P * 3 + R] = c * arp - s * arq
    A[R * 3 + Q] = A[Q * 3 + R] = s * arp + c * arq
    for r in range(3):
        vrp, vrq = V[r * 3 + P], V[r * 3 + Q]
        V[r * 3 + P] = c * vrp - s * vrq
        V[r * 3 + Q] = s * vrp + c * vrq


def jacobi3(A):
    """A: nine floats, row-major symmetric -> the three eigenvalues, unsorted (w[k] = A[k][k] at the end)"""
    A = [float(v) for v in A]
    V = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(32):
        if A[1] == 0.0 and A[2] == 0.0 and A[5] == 0.0:
            break
        _rotate(A, V, 0, 1)
        _rotate(A, V, 0, 2)
        _rotate(A, V, 1, 2)
    return [A[0], A[4], A[8]]


def _finite(v):
    return v - v == 0.0


def _div(a, b):
    """IEEE a / b for Python floats"""
    if b == 0.0:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def third_from_sums(sums, n_s, x, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """sums: six integers (xx xy xz yy yz zz) -> third (Python float)"""
    if n_s < min_neighbors:
        return 0.0
    xx, xy, xz, yy, yz, zz = [float(int(v)) for v in sums]  # (int -> double rounds to nearest, ties to even)
    l1, l2, l3 = jacobi3([xx, xy, xz, xy, yy, yz, xz, yz, zz])
    if l1 < l2:
        l1, l2 = l2, l1
    if l2 < l3:
        l2, l3 = l3, l2
    if l1 < l2:
        l1, l2 = l2, l1
    if not (_finite(l1) and _finite(l2) and _finite(l3)):
        return 0.0
    if not l3 > 0.0:
        return 0.0
    if not _div(l2, l1) < gamma_21:
        return 0.0
    if not _div(l3, l2) < gamma_32:
        return 0.0
    return math.ldexp(l3, x - SCALE_BITS)


# ---- the pairs

def _prep(cloud):
    cloud = np.ascontiguousarray(np.asarray(cloud)[:, :3], F)
    finite = np.isfinite(cloud).all(1)
    cand = np.nonzero(finite)[0]
    return cloud, finite, cand, cloud[cand]


def _d2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    d2 = (dx * dx + dy * dy) + dz * dz  # float32 arrays: every operation rounded, none fused
    assert d2.dtype == F
    return d2


def _terms(pi, pj, scale):
    """the six integer terms of neighbour j for point i, int64 [m, 6]"""
    d = (pj - pi)
    assert d.dtype == F
    d = d.astype(np.float64)
    prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                     d[:, 2] * d[:, 2]], axis=1)
    t = np.rint(prod * scale)  # (ties to even; the scaling by a power of two is exact)
    assert np.all(np.abs(t) < 2.0 ** 40)
    return t.astype(np.int64)


def _finish(n, finite, cand, sums, n_s, x, nms_count, nms_max, gamma_21, gamma_32, min_neighbors, third=None):
    """sums: per finite point six Python ints or an int64 row; nms_count / nms_max: functions of the third array ->
    per finite point the neighbours within r2n and the largest third among them"""
    m = len(cand)
    if third is None:
        third = np.array([third_from_sums(sums[i], int(n_s[i]), x, gamma_21, gamma_32, min_neighbors) for i in range(m)],
                         np.float64).reshape(m)
    cnt = nms_count()
    big = nms_max(third)
    salient = third > 0
    key = salient & (cnt >= min_neighbors) & ~(big > third)
    labels = np.zeros(n, np.uint8)
    labels[cand] = np.where(key, KEYPOINT, np.where(salient, SALIENT, PLAIN))
    third_c = np.zeros(n, np.float64)
    third_c[cand] = third
    counts = np.full(n, -1, np.int32)
    counts[cand] = n_s
    return dict(indices=np.nonzero(labels == KEYPOINT)[0].astype(np.int32), labels=labels, third=third_c, counts=counts,
                n_finite=m, n_salient=int(salient.sum()), n_keypoints=int(key.sum()), x=x,
                sums=np.array([[int(v) for v in s] for s in sums], np.int64).reshape(m, 6), finite=finite)


def keypoints_brute(cloud, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, chunk=256):
    """Every pair of finite points; the sums are Python integers."""
    cloud, finite, cand, c = _prep(cloud)
    r2s, r2n = r2_of(salient_radius), r2_of(non_max_radius)
    x = exponent_of(r2s)
    scale = math.ldexp(1.0, SCALE_BITS - x)
    m = len(cand)
    sums, n_s, near = [], np.zeros(m, np.int64), []
    for s in range(0, m, chunk):
        q = c[s:s + chunk]
        d2 = _d2(q[:, None, :], c[None, :, :])
        for a in range(len(q)):
            nb = np.nonzero(d2[a] < r2s)[0]
            t = _terms(np.broadcast_to(q[a], (len(nb), 3)), c[nb], scale)
            sums.append([int(t[:, k].astype(object).sum()) if len(nb) else 0 for k in range(6)])  # Python integers
            n_s[s + a] = len(nb)
            near.append(np.nonzero(d2[a] < r2n)[0])

    def nms_count():
        return np.array([len(v) for v in near], np.int64).reshape(m)

    def nms_max(third):
        return np.array([third[v].max() if len(v) else 0.0 for v in near], np.float64).reshape(m)

    return _finish(len(cloud), finite, cand, sums, n_s, x, nms_count, nms_max, gamma_21, gamma_32, min_neighbors)


def _pairs_within(c, radius, r2):
    """ordered pairs (i, j), i != j, with float32 d2 < r2, from a float64 kd-tree's candidates"""
    from scipy.spatial import cKDTree
    if len(c) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pairs = cKDTree(c.astype(np.float64)).query_pairs(float(radius) * 1.001 + 1e-6, output_type="ndarray")
    ok = _d2(c[pairs[:, 0]], c[pairs[:, 1]]) < r2
    a, b = pairs[ok, 0].astype(np.int64), pairs[ok, 1].astype(np.int64)
    return np.r_[a, b], np.r_[b, a]


def _by_row(rows, m):
    order = np.argsort(rows, kind="stable")
    counts = np.bincount(rows, minlength=m)
    return order, counts


def keypoints(cloud, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """Candidate pairs from a float64 kd-tree, the float32 test on them, int64 numpy sums."""
    cloud, finite, cand, c = _prep(cloud)
    r2s, r2n = r2_of(salient_radius), r2_of(non_max_radius)
    x = exponent_of(r2s)
    scale = math.ldexp(1.0, SCALE_BITS - x)
    m = len(cand)
    self_in_s, self_in_n = int(r2s > 0), int(r2n > 0)  # (d2 = 0 < r2: always, the radii are positive)
    i, j = _pairs_within(c, salient_radius, r2s)
    sums = np.zeros((m, 6), np.int64)
    if len(i):
        np.add.at(sums, i, _terms(c[i], c[j], scale))  # (the point's own term is zero)
    n_s = np.bincount(i, minlength=m).astype(np.int64) + self_in_s
    a, b = _pairs_within(c, non_max_radius, r2n)

    def nms_count():
        return np.bincount(a, minlength=m).astype(np.int64) + self_in_n

    def nms_max(third):
        big = third.copy()  # (itself is among its neighbours)
        if len(a):
            np.maximum.at(big, a, third[b])
        return big

    return _finish(len(cloud), finite, cand, sums, n_s, x, nms_count, nms_max, gamma_21, gamma_32, min_neighbors)


# ---- PCL as it is written (float64)

def pcl_literal(cloud, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """keypoints/impl/iss_3d.hpp in float64: getScatterMatrix adds the outer products of (p_j - p_i) in double in the
    list's order (here ascending index), SelfAdjointEigenSolver's values are numpy.linalg.eigvalsh's, and
    detectKeypoints applies e2 / e1 < gamma_21 && e3 / e2 < gamma_32 and the `<` test of the suppression.  The
    neighbourhoods are the rule's (float32 d2 < r2).  -> dict with salient / key [m] bool over the finite points,
    third, ratios (r21, r32), and the r2n neighbour pairs (a, b)."""
    cloud, finite, cand, c = _prep(cloud)
    r2s, r2n = r2_of(salient_radius), r2_of(non_max_radius)
    m = len(cand)
    i, j = _pairs_within(c, salient_radius, r2s)
    d = (c[j] - c[i]).astype(np.float64)
    order = np.lexsort((j, i))
    i, d = i[order], d[order]
    cov = np.zeros((m, 3, 3))
    n_s = np.bincount(i, minlength=m) + 1
    start = np.r_[0, np.cumsum(np.bincount(i, minlength=m))]
    outer = d[:, :, None] * d[:, None, :]
    for p in range(m):
        acc = np.zeros((3, 3))
        for k in range(start[p], start[p + 1]):  # list order, double
            acc += outer[k]
        cov[p] = acc
    ev = np.linalg.eigvalsh(cov)  # ascending
    e1, e2, e3 = ev[:, 2], ev[:, 1], ev[:, 0]
    with np.errstate(all="ignore"):
        r21, r32 = e2 / e1, e3 / e2
    ok = (n_s >= min_neighbors) & np.isfinite(ev).all(1) & (e3 >= 0)
    third = np.where(ok & (r21 < gamma_21) & (r32 < gamma_32), e3, 0.0)
    a, b = _pairs_within(c, non_max_radius, r2n)
    cnt = np.bincount(a, minlength=m) + 1
    big = third.copy()
    if len(a):
        np.maximum.at(big, a, third[b])
    salient = third > 0
    key = salient & (cnt >= min_neighbors) & ~(third < big)
    return dict(cand=cand, salient=salient, key=key, third=third, r21=r21, r32=r32, a=a, b=b, n_s=n_s, e=ev)


def compare_with_literal(ref, lit, gamma_21=0.975, gamma_32=0.975, rel=1e-6):
    """-> (differences not excused, points left out).  A point may be left out only when a decision of its own lies
    within `rel` relative of its bound: a ratio against its gamma, or its third against a neighbour's."""
    cand = lit["cand"]
    m = len(cand)
    sal_r = ref["labels"][cand] >= SALIENT
    key_r = ref["labels"][cand] == KEYPOINT
    with np.errstate(all="ignore"):
        near_gamma = (np.abs(lit["r21"] - gamma_21) <= rel * gamma_21) | (np.abs(lit["r32"] - gamma_32) <= rel * gamma_32)
    t = lit["third"]
    a, b = lit["a"], lit["b"]
    close = (t[a] > 0) & (t[b] > 0) & (t[a] != t[b]) & (np.abs(t[a] - t[b]) <= rel * np.abs(t[a]))
    near_nms = np.zeros(m, bool)
    near_nms[a[close]] = True
    excused = near_gamma | near_nms
    differ = (sal_r != lit["salient"]) | (key_r != lit["key"])
    return int((differ & ~excused).sum()), int((differ & excused).sum())


# ---- the cases of the tests

def median_spacing(cloud):
    from scipy.spatial import cKDTree
    c = _prep(cloud)[3].astype(np.float64)
    return float(np.median(cKDTree(c).query(c, 2)[0][:, 1]))


_CASES = None


def base_cases():
    """name -> (cloud, salient_radius, non_max_radius): fpfh_reference.clouds() at (1.0, 0.5) and at (6 x, 4 x the
    median spacing).  Built once."""
    global _CASES
    if _CASES is None:
        import fpfh_reference as FR
        out = {}
        for name, c in FR.clouds().items():
            s = median_spacing(c)
            out[name + "-1.0"] = (c, 1.0, 0.5)
            out[name + "-6x"] = (c, 6.0 * s, 4.0 * s)
        _CASES = out
    return _CASES


_REFS = {}


def reference(name):
    """keypoints(...) of a base case, computed once and shared"""
    if name not in _REFS:
        c, rs, rn = base_cases()[name]
        _REFS[name] = keypoints(c, rs, rn)
    return _REFS[name]


BIG_N, BIG_SEED, BIG_RADII = 20000, 42, (1.86, 1.24)
_BIG = None


def big_case():
    global _BIG
    if _BIG is None:
        from libwave_amd import synth
        cloud = np.ascontiguousarray(np.asarray(synth.scene(BIG_N, seed=BIG_SEED))[:, :3], F)
        _BIG = (cloud, keypoints(cloud, *BIG_RADII))
    return _BIG


def dense_cloud(n, seed=3):
    """n points uniform in a cube whose side keeps about 30 points inside a unit ball (the sizes around a wave)"""
    side = max((n * 4.19 / 30.0) ** (1.0 / 3.0), 1.0)
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0, side, (n, 3)), F)


def lattice(nx=12, ny=12, h=0.25):
    """an exact planar lattice (z = 0, spacing a power of two): l3 == 0 everywhere"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2) * h
    return np.ascontiguousarray(np.c_[g, np.zeros(len(g))], F)


def variants():
    """the other clouds of the device test: name -> (cloud, rs, rn, kwargs)"""
    d = dense_cloud(193)
    out = {"dense-%d" % n: (d[:n], 1.0, 0.6, {}) for n in (1, 2, 5, 63, 64, 65, 193)}
    scan = base_cases()["scan-1.0"][0]
    sub = scan[:1500]
    bad = sub.copy()
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    out["nan-inf"] = (bad, 1.0, 0.5, {})
    out["all-nan"] = (np.full((70, 3), np.nan, F), 1.0, 0.5, {})
    out["duplicate"] = (np.r_[sub, sub], 1.0, 0.5, {})
    out["far"] = ((sub.astype(np.float64) + 1.0e5).astype(F), 1.0, 0.5, {})
    out["whole-cloud-nms"] = (sub, 1.0, 500.0, {})
    out["lattice"] = (lattice(), 0.8, 0.5, {})
    out["gamma-0"] = (sub, 1.0, 0.5, dict(gamma_21=0.0, gamma_32=0.0))
    out["min-neighbors-high"] = (sub, 1.0, 0.5, dict(min_neighbors=100000))
    out["all-salient-kept"] = (sub, 1.0, 1e-4, dict(min_neighbors=1))
    return out
