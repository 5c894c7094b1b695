"""The checker of wm_sac_segment (include/wavematch.h, "plane segmentation"): PCL 1.8's RANSAC plane segmentation as
the header restates it, in numpy float32, with no project code in it.  Two forms:

  run_literal   one hypothesis at a time, the loop exactly as the header writes it;
  run_blocks    the stream evaluated in blocks (samples, planes and counts vectorised), the blocks walked in order.

tests/test_sac_reference_cpu.py holds the two equal on every case and pins the table of the cases.  Every float32
operation is a numpy float32 operation of its own (rounded, nothing fused); sqrt and the division are correctly
rounded in numpy as on the device."""
import math
import sys

import numpy as np

import knn_reference as KR

PLANE, PERPENDICULAR, PARALLEL = 0, 1, 2
NONE, INLIER, OUTLIER = 0, 1, 2
OK, NOT_CONVERGED = 0, 1
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
F = np.float32


# ------------------------------------------------------------------ the stream
def sm64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def r(seed, j, a, m):
    return ((sm64(seed + GOLD * (3 * j + a + 1)) >> 32) * m) >> 32


def sample(seed, j, n):
    i0 = r(seed, j, 0, n)
    t = r(seed, j, 1, n - 1)
    i1 = t + (t >= i0)
    t = r(seed, j, 2, n - 2)
    t += t >= min(i0, i1)
    t += t >= max(i0, i1)
    return i0, i1, t


def _sm64_v(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def samples_block(seed, j0, count, n):
    """entries j0 ... j0 + count - 1 -> int64 [count, 3]"""
    j = np.arange(j0, j0 + count, dtype=np.uint64)

    def rv(a, m):
        with np.errstate(over="ignore"):
            h = _sm64_v(np.uint64(seed & M64) + np.uint64(GOLD) * (np.uint64(3) * j + np.uint64(a + 1)))
        return (((h >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)

    i0 = rv(0, n)
    t = rv(1, n - 1)
    i1 = t + (t >= i0)
    t = rv(2, n - 2)
    t = t + (t >= np.minimum(i0, i1))
    t = t + (t >= np.maximum(i0, i1))
    return np.stack([i0, i1, t], 1)


# ------------------------------------------------------------------ planes, counts
def planes_of(P, idx):
    """idx int [m, 3] -> (coefficients float32 [m, 4], ok bool [m]); a skipped entry's row is zero"""
    with np.errstate(all="ignore"):
        p0, p1, p2 = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
        u = p1 - p0
        v = p2 - p0
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        s = (cx * cx + cy * cy) + cz * cz
        ok = np.isfinite(s) & (s > 0)
        l = np.sqrt(s)
        a, b, c = cx / l, cy / l, cz / l
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
        out = np.stack([a, b, c, d], 1).astype(F)
    out[~ok] = 0
    return out, ok


def plane(P, i0, i1, i2):
    out, ok = planes_of(P, np.array([[i0, i1, i2]]))
    return out[0] if ok[0] else None


def thr_f(t):
    """the smallest float32 not below t"""
    x = F(t)
    return x if float(x) >= t else np.nextafter(x, F(np.inf))


def axis_consts(axis, eps_angle):
    ax, ay, az = (float(v) for v in axis)
    l = math.sqrt((ax * ax + ay * ay) + az * az)
    return np.array([ax / l, ay / l, az / l]).astype(F), F(math.cos(eps_angle)), F(math.sin(eps_angle))


def axis_valid(pl, model, axis, eps_angle):
    """pl float32 [m, 4] -> bool [m]"""
    if model == PLANE:
        return np.ones(len(pl), bool)
    a, ce, se = axis_consts(axis, eps_angle)
    dot = np.abs((pl[:, 0] * a[0] + pl[:, 1] * a[1]) + pl[:, 2] * a[2])
    return dot >= ce if model == PERPENDICULAR else dot < se


def inliers(P, pl, th):
    """bool [n]: dist < th, a non-finite point never"""
    with np.errstate(all="ignore"):
        d = np.abs(((pl[0] * P[:, 0] + pl[1] * P[:, 1]) + pl[2] * P[:, 2]) + pl[3])
        return d < th


def counts_of(P, pls, th, chunk=1 << 22):
    out = np.zeros(len(pls), np.int64)
    step = max(1, chunk // max(len(P), 1))
    x, y, z = P[:, 0][None], P[:, 1][None], P[:, 2][None]
    with np.errstate(all="ignore"):
        for a in range(0, len(pls), step):
            q = pls[a:a + step]
            d = np.abs(((q[:, 0:1] * x + q[:, 1:2] * y) + q[:, 2:3] * z) + q[:, 3:4])
            out[a:a + step] = (d < th).sum(1)
    return out


# ------------------------------------------------------------------ the loop, two forms
class _Walk:
    """PCL's loop state; feed() takes one entry (skipped / axis-valid / count / plane), returns False when it ends."""

    def __init__(self, n, max_it, prob):
        self.n, self.max_it, self.max_skip = n, max_it, 10 * max_it
        self.log_p = math.log(1.0 - prob)
        self.it = self.skipped = self.j = self.axis_invalid = 0
        self.k, self.best, self.best_j, self.pl = 1.0, -1, -1, None

    def _k(self, count):
        eps = sys.float_info.epsilon
        q = 1.0 - (count / self.n) ** 3
        q = max(eps, min(1.0 - eps, q))
        return self.log_p / math.log(q)

    def going(self):
        return self.it < self.k and self.skipped < self.max_skip

    def feed(self, ok, valid, count, pl):
        j = self.j
        self.j += 1
        if not ok:
            self.skipped += 1
            return self.going()
        if not valid:
            self.axis_invalid += 1
            if self.best < 0:  # PCL: its count of 0 beats "nothing counted yet" and sets k -- but it is no model
                self.k = self._k(0)
        elif count > self.best:
            self.best, self.best_j, self.pl = int(count), j, pl.copy()
            self.k = self._k(count)
        self.it += 1
        if self.it > self.max_it:
            return False
        return self.going()

    def result(self):
        return dict(status=OK if self.best_j >= 0 else NOT_CONVERGED, iterations=self.it, skipped=self.skipped,
                    hypotheses=self.j, best_hypothesis=self.best_j, n_inliers_model=max(self.best, 0),
                    model_coefficients=self.pl, axis_invalid=self.axis_invalid)


def run_literal(P, thr, max_it=50, prob=0.99, seed=0, model=PLANE, axis=(0, 0, 1), eps_angle=0.0):
    """The header's loop, written out on its own (nothing shared with run_blocks' walk)."""
    n = len(P)
    it = skipped = j = axis_invalid = 0
    k, best, best_j, best_pl = 1.0, -1, -1, None
    if n >= 3:
        th = thr_f(thr)
        eps = sys.float_info.epsilon
        log_p = math.log(1.0 - prob)
        max_skip = 10 * max_it
        while it < k and skipped < max_skip:
            pl = plane(P, *sample(seed, j, n))
            j += 1
            if pl is None:
                skipped += 1
                continue
            if bool(axis_valid(pl[None], model, axis, eps_angle)[0]):
                count = int(inliers(P, pl, th).sum())
                if count > best:
                    best, best_j, best_pl = count, j - 1, pl
                    k = log_p / math.log(min(1.0 - eps, max(eps, 1.0 - (count / n) ** 3)))
            else:
                axis_invalid += 1
                if best < 0:  # the count 0 of PCL's countWithinDistance beats "nothing counted yet": k, but no model
                    k = log_p / math.log(1.0 - eps)
            it += 1
            if it > max_it:
                break
    return dict(status=OK if best_j >= 0 else NOT_CONVERGED, iterations=it, skipped=skipped, hypotheses=j,
                best_hypothesis=best_j, n_inliers_model=max(best, 0), model_coefficients=best_pl, axis_invalid=axis_invalid)


def run_blocks(P, thr, max_it=50, prob=0.99, seed=0, model=PLANE, axis=(0, 0, 1), eps_angle=0.0, block=256):
    n = len(P)
    w = _Walk(n, max_it, prob)
    if n < 3:
        return w.result()
    th = thr_f(thr)
    go = w.going()
    j0 = 0
    while go:
        pls, ok = planes_of(P, samples_block(seed, j0, block, n))
        valid = ok & axis_valid(pls, model, axis, eps_angle)
        cnt = np.zeros(block, np.int64)
        cnt[valid] = counts_of(P, pls[valid], th)
        for e in range(block):
            go = w.feed(bool(ok[e]), bool(valid[e]), int(cnt[e]), pls[e])
            if not go:
                break
        j0 += block
    return w.result()


# ------------------------------------------------------------------ selection, refit
def select(P, coef, thr):
    """-> (indices int32 ascending, labels uint8) of the plane `coef` (float32 [4])"""
    m = inliers(P, np.asarray(coef, F), thr_f(thr))
    labels = np.where(m, INLIER, np.where(np.isfinite(P).all(1), OUTLIER, NONE)).astype(np.uint8)
    return np.nonzero(m)[0].astype(np.int32), labels


def refit(P, model_pl, thr):
    """The float64 plane of the model's inliers -> dict(C, lam (ascending), n (unit, the sign of the model's normal),
    centroid, d) or None below 4 inliers."""
    Q = P[inliers(P, model_pl, thr_f(thr))].astype(np.float64)
    if len(Q) < 4:
        return None
    cen = Q.mean(0)
    D = Q - cen
    Cm = D.T @ D / len(Q)
    lam, vec = np.linalg.eigh(Cm)
    nv = vec[:, 0]
    if nv @ model_pl[:3].astype(np.float64) < 0:
        nv = -nv
    return dict(C=Cm, lam=lam, n=nv, centroid=cen, d=-(nv @ cen))


def segment(P, thr, optimize=True, **kw):
    """The whole call in the checker's own arithmetic -> run_blocks' dict + coefficients, indices, labels, refined."""
    out = run_blocks(P, thr, **kw)
    out.update(coefficients=None, indices=np.zeros(0, np.int32), labels=None, refined=0)
    if out["status"] != OK:
        return out
    coef = out["model_coefficients"]
    if optimize and out["n_inliers_model"] >= 4:
        f = refit(P, coef, thr)
        nf = f["n"].astype(F)
        longer = np.abs(nf.astype(np.float64)) > np.abs(f["n"])  # toward zero: never longer than the unit vector
        nf[longer] = np.nextafter(nf[longer], F(0))
        cand = np.r_[nf, F(-(nf.astype(np.float64) @ f["centroid"]))].astype(F)
        if np.isfinite(cand).all():
            coef, out["refined"] = cand, 1
    out["coefficients"] = coef
    out["indices"], out["labels"] = select(P, coef, thr)
    return out


# ------------------------------------------------------------------ the cases
def _decks():
    """dyadic lattice layers: z = 0 (32 x 32), 0.25 (32 x 16), -0.5 (16 x 16), spacing 0.25; the threshold is 0.25"""
    def layer(nx, ny, z):
        g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2) * 0.25
        return np.c_[g, np.full(len(g), z)]
    pts = np.r_[layer(32, 32, 0.0), layer(32, 16, 0.25), layer(16, 16, -0.5)]
    return np.ascontiguousarray(pts[np.random.default_rng(311).permutation(len(pts))], F)


SLAB_NORMAL = np.array([0.3, -0.2, 0.9327379053088815])  # (unit)


def _slab():
    """2000 points within 0.01 of a tilted plane through (1, 2, 3), 1000 uniform outliers"""
    rng = np.random.default_rng(312)
    nrm = SLAB_NORMAL / np.linalg.norm(SLAB_NORMAL)
    e1 = np.cross(nrm, [0, 0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    uv = rng.uniform(-10, 10, (2000, 2))
    on = np.array([1.0, 2.0, 3.0]) + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.uniform(-0.009, 0.009, (2000, 1)) * nrm
    pts = np.r_[on, rng.uniform(-10, 10, (1000, 3)) + [1.0, 2.0, 3.0]]
    return np.ascontiguousarray(pts[rng.permutation(3000)], F)


_OWN = None
OWN = ("decks", "slab")


def shapes():
    """knn_reference's shapes and the checker's own two (read-only)"""
    global _OWN
    if _OWN is None:
        _OWN = dict(KR.shapes(), decks=_decks(), slab=_slab())
        for c in _OWN.values():
            c.setflags(write=False)
    return _OWN


# (name, threshold, max_iterations, extra parameters): every case the GPU test holds the device to
CASES = [
    ("exact_plane", 0.05, 50, {}), ("line", 0.05, 50, {}), ("line", 0.5, 1000, {}), ("point", 0.05, 50, {}),
    ("point", 0.5, 1000, {}), ("scene", 0.05, 50, {}), ("scene", 0.05, 1000, {}), ("scene", 0.5, 50, {}),
    ("holes", 0.05, 50, {}), ("lattice", 0.5, 1000, {}), ("dups", 0.5, 1000, {}), ("shell", 0.5, 1000, {}),
    ("clumps_outliers", 0.05, 50, {}), ("noisy_plane", 0.05, 50, {}), ("utm_plane", 0.05, 50, {}),
    ("decks", 0.25, 50, {}), ("slab", 0.01, 50, {}),
    ("scene", 0.05, 50, dict(model=PERPENDICULAR, axis=(0, 0, 1), eps_angle=0.1)),
    ("scene", 0.05, 50, dict(model=PARALLEL, axis=(0, 0, 1), eps_angle=0.1)),
    ("scene", 0.05, 200, dict(model=PARALLEL, axis=(0, 0, 1), eps_angle=0.1)),
]

_CACHE = {}


def case(i, optimize=True):
    """segment() of CASES[i], computed once"""
    key = (i, optimize)
    if key not in _CACHE:
        name, thr, max_it, extra = CASES[i]
        _CACHE[key] = segment(shapes()[name], thr, optimize=optimize, max_it=max_it, **extra)
    return _CACHE[key]


def case_id(i):
    name, thr, max_it, extra = CASES[i]
    return "%s-%g-%d%s" % (name, thr, max_it, "-model%d" % extra["model"] if extra else "")
