"""The checker of wm_normals_radius and wm_fpfh_radius (libwave_amd/csrc/wm_fpfh_radius.hip): the rule of
include/wavematch.h ("feature descriptors", the radius forms) restated in numpy.  The pair features are
fpfh_reference's, the neighbour test and the integer terms are iss_reference's.

  neighbours  r2 = (float32) (radius * radius), the product in double; j is a neighbour of finite i iff d2 < r2
              (strict), i itself included; d2 = (dx * dx + dy * dy) + dz * dz in float32.  r2 = m 2^x, e = ceil(x / 2).
  normal      nine integer sums over the neighbours: rint(d_c 2^(36 - e)) and rint(d_a d_b 2^(36 - x)), d = p_j - p_i in
              float32, widened; mean and covariance from them in float64 (finish_from_sums: operation by operation as
              wm_normal_rule.hpp up to the covariance; the eigenvectors are numpy's, so the device's normal is held to
              it with plane_reference.check_normals' bars, and bit for bit to wm_normal_from_sums instead).
  SPFH        over the neighbours with 0 < d2 < r2 of the feature radius: fpfh_reference.pair_features.
  FPFH        W = rint((double) (r2 / max(d2, r2 2^-16)) 2^20), acc[b] += count_j[b] W in integers; per block
              out[b] = (float32) ((double) acc[b] * 100.0 / (double) total).
  two forms   the kd-tree variant (candidate pairs from a float64 kd-tree, the float32 test re-formed on them, int64
              numpy sums) and a brute-force one for small n (every pair, Python integers);
              tests/test_fpfh_radius_reference_cpu.py holds them to each other.
  pcl_literal PCL's own arithmetic in float64: double sums, 1 / d2 weights."""
import math

import numpy as np

import fpfh_reference as FR
import iss_reference as IR

F = np.float32
BINS, DIM = FR.BINS, FR.DIM
SCALE_BITS = 36
MAX_NEIGHBORS = 8191
WEIGHT_BITS = 20
CLAMP_BITS = 16


def half_exponent(x):
    """e = ceil(x / 2)"""
    return -((-int(x)) // 2)


def exponents(radius):
    r2 = IR.r2_of(radius)
    x = IR.exponent_of(r2)
    return r2, x, half_exponent(x)


# ---- the pairs

def _pairs_brute(c, r2):
    """ordered pairs (i, j), i != j, with float32 d2 < r2, every pair looked at"""
    m = len(c)
    if m < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    out_i, out_j = [], []
    for s in range(0, m, 256):
        d2 = IR._d2(c[s:s + 256, None, :], c[None, :, :])
        a, b = np.nonzero(d2 < r2)
        keep = (a + s) != b
        out_i.append(a[keep] + s)
        out_j.append(b[keep])
    return np.concatenate(out_i).astype(np.int64), np.concatenate(out_j).astype(np.int64)


def pairs(c, radius, brute=False):
    r2 = IR.r2_of(radius)
    return _pairs_brute(c, r2) if brute else IR._pairs_within(c, radius, r2)


def _segment_sum(values, rows, m):
    """exact int64 sums of `values` [p, k] per row id -> [m, k]"""
    out = np.zeros((m,) + values.shape[1:], np.int64)
    if len(rows) == 0:
        return out
    order = np.argsort(rows, kind="stable")
    r, v = rows[order], values[order]
    starts = np.r_[0, np.nonzero(np.diff(r))[0] + 1]
    out[r[starts]] = np.add.reduceat(v, starts, axis=0)
    return out


# ---- normals

def _normal_terms(pi, pj, x, e):
    d = pj - pi
    assert d.dtype == F
    d = d.astype(np.float64)
    s1, s2 = math.ldexp(1.0, SCALE_BITS - e), math.ldexp(1.0, SCALE_BITS - x)
    v = np.stack([d[:, 0] * s1, d[:, 1] * s1, d[:, 2] * s1, d[:, 0] * d[:, 0] * s2, d[:, 0] * d[:, 1] * s2, d[:, 0] * d[:, 2] * s2,
                  d[:, 1] * d[:, 1] * s2, d[:, 1] * d[:, 2] * s2, d[:, 2] * d[:, 2] * s2], axis=1)
    t = np.rint(v)  # (ties to even; the scaling by a power of two is exact)
    assert np.all(np.abs(t) < 2.0 ** 40)
    return t.astype(np.int64)


def normal_sums(cloud, radius, brute=False):
    """-> dict(sums [n, 9] int64 (x y z xx xy xz yy yz zz; zeros for a non-finite point), counts [n] int32 (n_s; -1 for
    a non-finite point), x, e, finite).  brute: every pair, the sums as Python integers."""
    cloud, finite, cand, c = IR._prep(cloud)
    r2, x, e = exponents(radius)
    m = len(cand)
    i, j = pairs(c, radius, brute)
    terms = _normal_terms(c[i], c[j], x, e) if len(i) else np.zeros((0, 9), np.int64)  # (the point's own terms are zero)
    if brute:
        acc = [[0] * 9 for _ in range(m)]
        for row, t in zip(i.tolist(), terms.tolist()):
            a = acc[row]
            for k in range(9):
                a[k] += t[k]
        assert all(abs(v) < 2 ** 63 for a in acc for v in a)
        s = np.array(acc, np.int64).reshape(m, 9)
    else:
        s = _segment_sum(terms, i, m)
    sums = np.zeros((len(cloud), 9), np.int64)
    sums[cand] = s
    counts = np.full(len(cloud), -1, np.int32)
    counts[cand] = np.bincount(i, minlength=m) + 1
    return dict(sums=sums, counts=counts, x=x, e=e, finite=finite)


def finish_from_sums(sums, counts, x, cloud):
    """The rule from the sums on, float64; the eigenvectors by numpy.linalg.eigh.  -> the dict plane_reference.
    check_normals takes as `ref`: normal [n, 3], curvature [n], gap [n], tie [n] (never), valid [n], and cov [n, 3, 3]."""
    sums = np.asarray(sums, np.int64)
    counts = np.asarray(counts)
    P = np.ascontiguousarray(np.asarray(cloud)[:, :3], F).astype(np.float64)
    n = len(sums)
    e = half_exponent(x)
    has = counts >= 3
    nn = np.where(has, counts, 1).astype(np.float64)
    q1, q2 = math.ldexp(1.0, e - SCALE_BITS), math.ldexp(1.0, x - SCALE_BITS)
    mean = sums[:, :3].astype(np.float64) * q1 / nn[:, None]
    sec = sums[:, 3:].astype(np.float64) * q2 / nn[:, None]
    cov = np.zeros((n, 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        cov[:, a, b] = cov[:, b, a] = sec[:, k] - mean[:, a] * mean[:, b]
    cov[~has] = np.eye(3)
    w, v = np.linalg.eigh(cov)  # ascending
    nrm = v[:, :, 0].copy()
    flip = np.einsum("na,na->n", nrm, np.where(np.isfinite(P), P, 0.0)) > 0
    nrm[flip] *= -1
    tot = w.sum(1)
    ok = has & (w[:, 2] > 0)
    curv = np.where(ok, w[:, 0] / np.where(tot > 0, tot, 1.0), 0.0)
    nrm[~ok] = 0.0
    # (a point without a normal is `not valid`, not `undetermined`: its gap is 1, and check_normals leaves it alone)
    gap = np.where(ok, (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], 1.0), 1.0)
    return dict(normal=nrm, curvature=curv, eig=w, gap=gap, tie=np.zeros(n, bool), valid=ok, cov=cov)


def normals(cloud, radius):
    """float32 [n, 4] records of the reference's own finish (numpy's eigenvectors: NOT the device's bits)"""
    s = normal_sums(cloud, radius)
    f = finish_from_sums(s["sums"], s["counts"], s["x"], cloud)
    return np.ascontiguousarray(np.c_[f["normal"], f["curvature"]], F), s, f


def pcl_normals_literal(cloud, radius):
    """pcl::NormalEstimation as it is written, float64: the neighbourhood's points (not differences) averaged and their
    covariance about the mean, doubles added in index order, numpy.linalg.eigh.  The neighbourhoods are the rule's.
    -> the dict check_normals takes."""
    cloud, finite, cand, c = IR._prep(cloud)
    m = len(cand)
    i, j = pairs(c, radius)
    i, j = np.r_[i, np.arange(m)], np.r_[j, np.arange(m)]
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    P = c.astype(np.float64)
    cnt = np.bincount(i, minlength=m)
    start = np.r_[0, np.cumsum(cnt)]
    cov = np.zeros((m, 3, 3))
    for p in range(m):
        nb = P[j[start[p]:start[p + 1]]] - P[p]  # (PCL's demeaned form; about the point itself the doubles stay small)
        mu = nb.mean(0)
        d = nb - mu
        cov[p] = d.T @ d / len(nb)
    has = cnt >= 3
    cov[~has] = np.eye(3)
    w, v = np.linalg.eigh(cov)
    nrm = v[:, :, 0].copy()
    flip = np.einsum("na,na->n", nrm, P) > 0
    nrm[flip] *= -1
    tot = w.sum(1)
    ok = has & (w[:, 2] > 0)
    n = len(cloud)

    def full(a, fill=0.0):
        out = np.full((n,) + a.shape[1:], fill, a.dtype)
        out[cand] = a
        return out

    curv = np.where(ok, w[:, 0] / np.where(tot > 0, tot, 1.0), 0.0)
    nrm[~ok] = 0.0
    gap = np.where(ok, (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], 1.0), 1.0)
    return dict(normal=full(nrm), curvature=full(curv), gap=full(gap, 1.0), tie=np.zeros(n, bool), valid=full(ok, False))


# ---- descriptors

def feature_pairs(cloud, radius, brute=False):
    """-> (cloud [n, 3] float32, finite [n], i, j, d2): the ordered pairs of CALLER indices with 0 < d2 < r2"""
    cloud, finite, cand, c = IR._prep(cloud)
    i, j = pairs(c, radius, brute)
    d2 = IR._d2(c[i], c[j]) if len(i) else np.zeros(0, F)
    keep = d2 != 0
    return cloud, finite, cand[i[keep]], cand[j[keep]], d2[keep]


def spfh(cloud, normals_, radius, brute=False, pairs_=None):
    """The first walk -> (counts [n, 33] int32, n_f [n] int32 (-1 for a non-finite point), f1_risky [n] int: pairs of
    the point whose f1 bin coordinate, computed in float64, lies within 1e-4 of an integer)."""
    cloud, finite, i, j, d2 = pairs_ if pairs_ is not None else feature_pairs(cloud, radius, brute)
    nrm = np.ascontiguousarray(np.asarray(normals_)[:, :3], F)
    n = len(cloud)
    counts = np.zeros((n, DIM), np.int32)
    n_f = np.where(finite, np.bincount(i, minlength=n), -1).astype(np.int32)
    risky = np.zeros(n, np.int64)
    if len(i):
        f = FR.pair_features(cloud[i], nrm[i], cloud[j], nrm[j])
        ok = f["ok"]
        for b in range(3):
            np.add.at(counts, (i[ok], b * BINS + f["bins"][:, b][ok]), 1)
        f64 = FR.pair_features(cloud[i], nrm[i], cloud[j], nrm[j], dtype=np.float64, swap=f["swap"])
        risky = np.bincount(i[ok & FR.near_integer(f64["x1"])], minlength=n)
    return counts, n_f, risky


def pair_weights(d2, r2):
    """W of the rule, int64"""
    with np.errstate(all="ignore"):
        floor = r2 * F(2.0 ** -CLAMP_BITS)
        assert floor.dtype == F
        ratio = r2 / np.maximum(d2, floor)
    assert ratio.dtype == F
    return np.rint(ratio.astype(np.float64) * float(1 << WEIGHT_BITS)).astype(np.int64)


def weight(counts, cloud, normals_, radius, brute=False, pairs_=None):
    """The second walk on given counts -> [n, 33] float32."""
    cloud, finite, i, j, d2 = pairs_ if pairs_ is not None else feature_pairs(cloud, radius, brute)
    nrm = np.ascontiguousarray(np.asarray(normals_)[:, :3], F)
    counts = np.asarray(counts).astype(np.int64)
    n = len(cloud)
    r2 = IR.r2_of(radius)
    valid = finite & ~np.all(nrm == 0, axis=1)
    W = pair_weights(d2, r2)
    if brute:
        acc_l = [[0] * DIM for _ in range(n)]
        for a, b, w in zip(i.tolist(), j.tolist(), W.tolist()):
            row, cj = acc_l[a], counts[b].tolist()
            for k in range(DIM):
                row[k] += cj[k] * w
        assert all(v < 2 ** 62 for row in acc_l for v in row)
        acc = np.array(acc_l, np.int64).reshape(n, DIM)
    else:
        acc = np.zeros((n, DIM), np.int64)
        for s in range(0, len(i), 1 << 18):  # (chunks: [pairs, 33] int64)
            acc += _segment_sum(counts[j[s:s + (1 << 18)]] * W[s:s + (1 << 18), None], i[s:s + (1 << 18)], n)
    out = np.zeros((n, DIM), F)
    for f in range(3):
        blk = acc[:, f * BINS:(f + 1) * BINS]
        total = blk.sum(axis=1)
        with np.errstate(all="ignore"):
            q = (blk.astype(np.float64) * 100.0) / total.astype(np.float64)[:, None]
        out[:, f * BINS:(f + 1) * BINS] = np.where(total[:, None] != 0, q, 0.0).astype(F)
    out[~valid] = 0
    return out


def fpfh(cloud, normals_, radius, brute=False):
    p = feature_pairs(cloud, radius, brute)
    counts, n_f, risky = spfh(cloud, normals_, radius, pairs_=p)
    return counts, weight(counts, cloud, normals_, radius, brute=brute, pairs_=p), n_f, risky


def pcl_weight_literal(counts, cloud, normals_, radius):
    """FPFHEstimation::weightPointSPFHSignature in float64 on given counts: weight 1 / d2, the sums in double, each
    block normalised to 100.  -> ([n, 33] float64, near [n]: the point has a neighbour with d2 < r2 2^-16)"""
    cloud, finite, i, j, d2 = feature_pairs(cloud, radius)
    nrm = np.ascontiguousarray(np.asarray(normals_)[:, :3], F)
    n = len(cloud)
    w = 1.0 / d2.astype(np.float64)
    acc = np.zeros((n, DIM))
    np.add.at(acc, i, np.asarray(counts)[j].astype(np.float64) * w[:, None])
    out = np.zeros((n, DIM))
    for f in range(3):
        blk = acc[:, f * BINS:(f + 1) * BINS]
        s = blk.sum(axis=1, keepdims=True)
        out[:, f * BINS:(f + 1) * BINS] = np.where(s != 0, blk * 100.0 / np.where(s != 0, s, 1.0), 0.0)
    out[~(finite & ~np.all(nrm == 0, axis=1))] = 0
    r2 = IR.r2_of(radius)
    near = np.bincount(i[d2 < r2 * F(2.0 ** -CLAMP_BITS)], minlength=n) > 0
    return out, near


# ---- the cases of the tests (built once, left unchanged)

RADII = (6, 10)  # feature radius in median spacings; the normal radius is half of it
# the largest share of points with an f1-risky pair over the three clouds, per radius, rounded up: measured with this
# reference alone (tests/test_fpfh_radius_reference_cpu.py: 1.00 / 0.25 / 1.53 % at 6 x, 1.43 / 0.27 / 1.72 % at 10 x)
RISKY_SHARE = {6: 0.016, 10: 0.018}
_SPACING = {}
_REFS = {}


def spacing(name):
    if name not in _SPACING:
        _SPACING[name] = IR.median_spacing(FR.clouds()[name])
    return _SPACING[name]


def radii(name, mult):
    """(normal_radius, feature_radius) of a cloud at `mult` median spacings"""
    s = spacing(name)
    return 0.5 * mult * s, float(mult) * s


def normal_reference(name, mult):
    """normal_sums of FR.clouds()[name] at the NORMAL radius of `mult`, computed once"""
    key = ("n", name, mult)
    if key not in _REFS:
        _REFS[key] = normal_sums(FR.clouds()[name], radii(name, mult)[0])
    return _REFS[key]


def dense_ball(n, radius=1.0, seed=11):
    """n distinct points inside a ball of `radius` / 2.2 about (3, 2, 1): each within `radius` of every other"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None] * (radius / 2.2)
    return np.ascontiguousarray(v + np.array([3.0, 2.0, 1.0]), F)
