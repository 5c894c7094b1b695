"""wm_cluster_boxes (libwave_amd/csrc/wm_describe.hip) restated in numpy and Python integers: the checker of
tests/test_boxes_gpu.py, in the manner of cluster_reference.py.  The rule is the one of include/wavematch.h ("cluster
boxes"):

  members   member e is record indices[e] (indices None: record e); cluster c is members [offsets[c], offsets[c + 1]).
            A non-finite member is skipped and sets NONFINITE; n counts the finite ones; n == 0 sets EMPTY.
  aabb      min / max of the floats by their orderable keys (-0 < +0), exact.
  sums      a = aabb_min in double; d = (double) p - a; the nine terms d.x d.y d.z d.x d.x d.x d.y d.x d.z d.y d.y d.y d.z
            d.z d.z in double, each entering as the integer trunc(t * 2^56); the integers added exactly.  A component
            of aabb_max - a of 2^20 or more sets RANGE (no sums).
  exact     `totals` are those integers (nine per cluster): what every form of the sum must agree on.
  moments   m = S1 / n, C = S2 / n - m m^T in float64 from S = total * 2^-56 (for the tolerance checks; the exact
            centroid a + total / (n 2^56) is a Fraction: centroid_exact).

Two forms: boxes() splits every term into three 40-bit limbs in int64 numpy arrays and adds them with
np.add.reduceat; boxes_slow() adds Python integers member by member.  tests/test_boxes_reference_cpu.py holds the two
to each other.  obb_from() restates the OBB arithmetic operation by operation on a given float32 centroid and axes."""
from fractions import Fraction

import numpy as np

EMPTY, NONFINITE, RANGE = 1, 2, 4
FLT_MIN = float(np.finfo(np.float32).tiny)
TERMS = [(0,), (1,), (2,), (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def key32(f):
    """float32 array -> uint32 whose unsigned order is the float order, -0 below +0"""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey32(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k >> np.uint32(31), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _members(points, offsets, indices):
    points = np.ascontiguousarray(points, np.float32)[:, :3]
    offsets = np.asarray(offsets).astype(np.int64)
    mem = points if indices is None else points[np.asarray(indices).astype(np.int64)]
    assert offsets[0] == 0 and offsets[-1] == len(mem) and (np.diff(offsets) >= 0).all()
    return mem, offsets


def _terms(d):
    """(m, 3) float64 -> (m, 9) float64: every product rounded once, as the device forms it"""
    return np.stack([d[:, t[0]] if len(t) == 1 else d[:, t[0]] * d[:, t[1]] for t in TERMS], axis=1)


def _limbs(t):
    """float64 t, 0 <= t < 2^63 -> three int64 arrays l0, l1, l2 with trunc(t * 2^56) = l2 2^80 + l1 2^40 + l0
    (wm_bins.hpp's bins_split: every step exact)"""
    t2 = np.trunc(t * 2.0 ** -24)
    r1 = t - t2 * 2.0 ** 24
    t1 = np.trunc(r1 * 2.0 ** 16)
    r0 = r1 - t1 * 2.0 ** -16
    t0 = np.trunc(r0 * 2.0 ** 56)
    return t0.astype(np.int64), t1.astype(np.int64), t2.astype(np.int64)


def _finish(n, flags, kmin, kmax, totals, a):
    """the shared tail: the structured fields from the counts, keys and exact totals"""
    C = len(n)
    out = dict(n=n.astype(np.uint32), flags=flags.astype(np.uint32), totals=totals)
    has = n > 0
    out["aabb_min"] = np.where(has[:, None], unkey32(kmin.reshape(-1)).reshape(C, 3), np.float32(0)).astype(np.float32)
    out["aabb_max"] = np.where(has[:, None], unkey32(kmax.reshape(-1)).reshape(C, 3), np.float32(0)).astype(np.float32)
    S = totals.astype(np.float64).reshape(C, 9) * 2.0 ** -56  # (a Python int -> float is rounded once, to nearest)
    nd = np.maximum(n, 1).astype(np.float64)[:, None]
    m = S[:, :3] / nd
    cov = np.zeros((C, 3, 3))
    for j, t in enumerate(TERMS[3:], 3):
        cov[:, t[0], t[1]] = cov[:, t[1], t[0]] = S[:, j] / nd[:, 0] - m[:, t[0]] * m[:, t[1]]
    live = has & ((flags & RANGE) == 0)
    out["mean"] = np.where(live[:, None], m, 0.0)
    out["cov"] = np.where(live[:, None, None], cov, 0.0)
    out["mu"] = np.linalg.eigvalsh(out["cov"])[:, ::-1] if C else np.zeros((0, 3))  # descending
    out["a"] = a
    return out


def boxes(points, offsets, indices=None):
    """The fast form -> dict of per-cluster arrays: n, flags, aabb_min, aabb_max (what the device must return bit for
    bit), totals (object array (C, 9) of Python ints), mean / cov / mu (float64) and a (aabb_min in float64)."""
    mem, offsets = _members(points, offsets, indices)
    C = len(offsets) - 1
    size = np.diff(offsets)
    cid = np.repeat(np.arange(C), size)
    finite = np.isfinite(mem).all(1)
    k = key32(mem.reshape(-1)).reshape(-1, 3)
    kmin_m = np.where(finite[:, None], k, np.uint32(0xFFFFFFFF))
    kmax_m = np.where(finite[:, None], k, np.uint32(0))
    ne = np.nonzero(size > 0)[0]          # reduceat over the non-empty clusters: their starts are strictly ascending
    starts = offsets[:-1][ne]
    n = np.zeros(C, np.int64)
    nonf = np.zeros(C, np.int64)
    kmin = np.full((C, 3), 0xFFFFFFFF, np.uint32)
    kmax = np.zeros((C, 3), np.uint32)
    if len(ne):
        n[ne] = np.add.reduceat(finite.astype(np.int64), starts)
        nonf[ne] = np.add.reduceat((~finite).astype(np.int64), starts)
        kmin[ne] = np.minimum.reduceat(kmin_m, starts, axis=0)
        kmax[ne] = np.maximum.reduceat(kmax_m, starts, axis=0)
    flags = np.where(n == 0, EMPTY, 0) | np.where(nonf > 0, NONFINITE, 0)
    a = np.where((n > 0)[:, None], unkey32(kmin.reshape(-1)).reshape(C, 3).astype(np.float64), 0.0)
    hi = np.where((n > 0)[:, None], unkey32(kmax.reshape(-1)).reshape(C, 3).astype(np.float64), 0.0)
    flags = flags | np.where(((hi - a) >= 2.0 ** 20).any(1), RANGE, 0)
    use = finite & ((flags[cid] & RANGE) == 0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(use[:, None], mem.astype(np.float64) - a[cid], 0.0)
    t = _terms(d)
    assert (t >= 0).all() and (t < 2.0 ** 40).all()
    l0, l1, l2 = _limbs(t)
    L = np.zeros((3, C, 9), np.int64)     # a limb is below 2^40: 2^23 members fit an int64
    if len(ne):
        for i, l in enumerate((l0, l1, l2)):
            L[i][ne] = np.add.reduceat(l, starts, axis=0)
    totals = (L[2].astype(object) << 80) + (L[1].astype(object) << 40) + L[0].astype(object)
    return _finish(n, flags, kmin, kmax, totals, a)


def boxes_slow(points, offsets, indices=None):
    """The slow form: every comparison and every sum in Python, member by member."""
    mem, offsets = _members(points, offsets, indices)
    C = len(offsets) - 1
    n = np.zeros(C, np.int64)
    flags = np.zeros(C, np.int64)
    kmin = np.full((C, 3), 0xFFFFFFFF, np.uint32)
    kmax = np.zeros((C, 3), np.uint32)
    totals = np.zeros((C, 9), object)
    a = np.zeros((C, 3))
    for c in range(C):
        rows = [p for p in mem[offsets[c]:offsets[c + 1]]]
        fin = [p for p in rows if np.isfinite(p).all()]
        n[c] = len(fin)
        if len(fin) < len(rows):
            flags[c] |= NONFINITE
        if not fin:
            flags[c] |= EMPTY
            continue
        keys = [[int(v) for v in key32(p)] for p in fin]
        kmin[c] = [min(k[i] for k in keys) for i in range(3)]
        kmax[c] = [max(k[i] for k in keys) for i in range(3)]
        a[c] = unkey32(kmin[c]).astype(np.float64)
        if ((unkey32(kmax[c]).astype(np.float64) - a[c]) >= 2.0 ** 20).any():
            flags[c] |= RANGE
            continue
        tot = [0] * 9
        for p in fin:
            d = [float(np.float64(p[i]) - a[c][i]) for i in range(3)]
            for j, t in enumerate(TERMS):
                v = d[t[0]] if len(t) == 1 else d[t[0]] * d[t[1]]  # (a Python float product: one rounding)
                num, den = v.as_integer_ratio()
                tot[j] += (num << 56) // den                       # trunc(v * 2^56), exactly (v >= 0)
        totals[c] = tot
    return _finish(n, flags, kmin, kmax, totals, a)


def centroid_exact(ref, c):
    """the three exact rationals a + total / (n 2^56) of cluster c"""
    n = int(ref["n"][c])
    return [Fraction(float(ref["a"][c][i])) + Fraction(int(ref["totals"][c][i]), n << 56) for i in range(3)]


def centroid_within_one_ulp(ref, got):
    """per cluster: is every component of the float32 centroid `got` within one float32 ulp (its own spacing) of the
    exact rational?  A float64 estimate settles the clear cases (its error bounded explicitly), Fractions the rest."""
    got = np.asarray(got, np.float32)
    live = (ref["n"] > 0) & ((ref["flags"] & RANGE) == 0)
    ulp = np.spacing(np.abs(got)).astype(np.float64)
    est = ref["a"] + ref["mean"]
    est_err = 2.0 ** -50 * (np.abs(ref["a"]) + np.abs(ref["mean"]))
    diff = np.abs(got.astype(np.float64) - est)
    clear = (diff <= 0.75 * ulp) & (est_err <= 0.125 * ulp)
    ok = clear.copy()
    for c, i in zip(*np.nonzero(~clear & live[:, None])):
        ok[c, i] = abs(Fraction(float(got[c, i])) - centroid_exact(ref, c)[i]) <= Fraction(float(ulp[c, i]))
    return ok.all(1) | ~live


def obb_from(points, centroid_f32, axes_f32):
    """PCL's computeOBB on the finite rows of `points` (one cluster's members), operation by operation:
    -> (obb_center float32 [3], obb_half float32 [3])"""
    p = np.ascontiguousarray(points, np.float32)[:, :3]
    p = p[np.isfinite(p).all(1)].astype(np.float64)
    cen = np.asarray(centroid_f32, np.float32).astype(np.float64)
    ax = np.asarray(axes_f32, np.float32).astype(np.float64).reshape(3, 3)
    e = p - cen
    mid, half = [], []
    for k in range(3):
        s = (e[:, 0] * ax[k, 0] + e[:, 1] * ax[k, 1]) + e[:, 2] * ax[k, 2]
        lo, hi = s.min(), s.max()
        half.append(np.float32((hi - lo) / 2.0))
        mid.append((hi + lo) / 2.0)
    center = [np.float32(((cen[i] + mid[0] * ax[0, i]) + mid[1] * ax[1, i]) + mid[2] * ax[2, i]) for i in range(3)]
    return np.array(center, np.float32), np.array(half, np.float32)


def check_properties(ref, box, points, offsets, indices=None, clusters=None):
    """The tolerance checks of a boxes array `box` (fields of wm_cluster_box) against the checker's `ref`, for the
    clusters given (default: all).  Bounds: float32 output rounding, 2^-25 relative per component, times at most 4:
      eigenvalues   |l_k - mu_k| <= 2^-22 mu_max + FLT_MIN; descending, >= 0
      axes          |a_i . a_j - delta_ij| <= 2^-21; det > 0; the sign rule on major and middle
      residual      |C a_k - l_k a_k| <= 2^-21 mu_max + FLT_MIN
      containment   |(p - obb_center) . a_k| <= obb_half[k] + 2^-20 (obb_half[k] + |obb_center|) for every member, and
                    each face has a member within that margin of it
    -> the number of clusters checked."""
    mem, offsets = _members(points, offsets, indices)
    assert centroid_within_one_ulp(ref, box["centroid"]).all()
    live = (ref["n"] > 0) & ((ref["flags"] & RANGE) == 0)
    for f in ("centroid", "eigenvalues", "axes", "obb_center", "obb_half"):  # nothing but zeros elsewhere
        assert not box[f][~live].view(np.uint32).any(), f
    # every live cluster at once
    lam = box["eigenvalues"][live].astype(np.float64)
    axf = box["axes"][live].reshape(-1, 3, 3)
    ax = axf.astype(np.float64)
    mu, cov = ref["mu"][live], ref["cov"][live]
    mu_max = np.maximum(mu[:, 0], 0.0)
    assert (np.abs(lam - np.maximum(mu, 0.0)) <= (2.0 ** -22 * mu_max + FLT_MIN)[:, None]).all()
    assert (lam[:, 0] >= lam[:, 1]).all() and (lam[:, 1] >= lam[:, 2]).all() and (lam[:, 2] >= 0.0).all()
    assert (np.abs(ax @ ax.transpose(0, 2, 1) - np.eye(3)) <= 2.0 ** -21).all()
    assert (np.linalg.det(ax) > 0).all()
    for k in range(2):  # the sign rule (argmax: the lowest index on ties)
        big = np.argmax(np.abs(axf[:, k]), axis=1)
        assert (np.take_along_axis(axf[:, k], big[:, None], 1)[:, 0] > 0).all(), k
    assert (ax[lam[:, 0] == 0.0] == np.eye(3)).all()
    for k in range(3):
        r = np.einsum("cij,cj->ci", cov, ax[:, k]) - lam[:, k, None] * ax[:, k]
        assert (np.linalg.norm(r, axis=1) <= 2.0 ** -21 * mu_max + FLT_MIN).all(), k
    # containment, cluster by cluster
    done = 0
    for c in (np.nonzero(live)[0] if clusters is None else clusters):
        if not live[c]:
            continue
        b = box[c]
        axc = np.asarray(b["axes"], np.float32).astype(np.float64).reshape(3, 3)
        p = mem[offsets[c]:offsets[c + 1]]
        p = p[np.isfinite(p).all(1)].astype(np.float64)
        cen, half = b["obb_center"].astype(np.float64), b["obb_half"].astype(np.float64)
        s = (p - cen) @ axc.T
        margin = 2.0 ** -20 * (half + np.linalg.norm(cen))
        assert (np.abs(s) <= half + margin).all(), (c, np.abs(s).max(0), half)
        assert (s.max(0) >= half - margin).all() and (s.min(0) <= -half + margin).all(), c
        done += 1
    return done


def check_exact(ref, box, points, offsets, indices=None, clusters=None):
    """The bit-for-bit checks: n, flags, aabb, reserved against the checker; obb_half / obb_center against obb_from on
    the box's OWN centroid and axes."""
    mem, offsets = _members(points, offsets, indices)
    assert np.array_equal(box["n"], ref["n"])
    assert np.array_equal(box["flags"], ref["flags"]), np.nonzero(box["flags"] != ref["flags"])
    for f in ("aabb_min", "aabb_max"):
        assert np.array_equal(box[f].view(np.uint32), ref[f].view(np.uint32)), f
    assert not box["reserved"].any()
    for c in (range(len(ref["n"])) if clusters is None else clusters):
        if ref["n"][c] == 0 or ref["flags"][c] & RANGE:
            continue
        center, half = obb_from(mem[offsets[c]:offsets[c + 1]], box["centroid"][c], box["axes"][c])
        assert np.array_equal(center.view(np.uint32), box["obb_center"][c].view(np.uint32)), (c, center, box["obb_center"][c])
        assert np.array_equal(half.view(np.uint32), box["obb_half"][c].view(np.uint32)), (c, half, box["obb_half"][c])


def as_box_array(ref, dtype):
    """The checker's own boxes as a structured array (axes by numpy's eigh under the rule's order and signs): what the
    property checks are first tried on, without a device."""
    C = len(ref["n"])
    out = np.zeros(C, dtype)
    out["n"], out["flags"] = ref["n"], ref["flags"]
    out["aabb_min"], out["aabb_max"] = ref["aabb_min"], ref["aabb_max"]
    for c in range(C):
        if ref["n"][c] == 0 or ref["flags"][c] & RANGE:
            continue
        out["centroid"][c] = [np.float32(float(v)) for v in centroid_exact(ref, c)]
        w, v = np.linalg.eigh(ref["cov"][c])
        w, v = np.maximum(w[::-1], 0.0), v[:, ::-1].T  # rows: major, middle, minor
        if w[0] == 0.0:
            v = np.eye(3)
        for k in range(2):
            f = np.abs(v[k].astype(np.float32))
            if v[k][int(np.argmax(f))] < 0:
                v[k] = -v[k]
        v[2] = np.cross(v[0], v[1])
        out["eigenvalues"][c], out["axes"][c] = w.astype(np.float32), v.astype(np.float32)
    return out


def fill_obb(box, points, offsets, indices=None):
    mem, offsets = _members(points, offsets, indices)
    for c in range(len(box)):
        if box["n"][c] and not box["flags"][c] & RANGE:
            box["obb_center"][c], box["obb_half"][c] = obb_from(mem[offsets[c]:offsets[c + 1]], box["centroid"][c],
                                                                box["axes"][c])
    return box
