"""The checker of wm_fpfh_estimate and wm_feature_match: the rule of include/wavematch.h ("feature descriptors")
restated in numpy float32, operation by operation, and beside it a literal float64 restatement of PCL 1.8's formulae
(features/impl/pfh_tools.hpp computePairFeatures, features/impl/fpfh.hpp) that tests/test_fpfh_reference_cpu.py pins
the rule to, pair by pair.  Everything is vectorised over pairs; nothing here sums with np.sum (pairwise) where the
rule states an order."""
import numpy as np

F = np.float32
BINS = 11
DIM = 33
PI32 = F(np.pi)
INV2PI32 = F(1.0 / (2.0 * np.pi))
AMBIGUOUS_EPS = 1e-4


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _bin(x, dtype):
    with np.errstate(invalid="ignore"):
        return np.clip(np.floor(dtype(BINS) * x), 0, BINS - 1)


def pair_features(p, n_p, q, n_q, dtype=F, swap=None, pcl=False):
    """The pair features of (p, q), arrays [..., 3] -> dict(ok, swap, a1, a2, f1, f2, f3, x1, x2, x3, bins [..., 3]).
    dtype = float32: the rule (x1..x3 are the bin coordinates before floorf).  dtype = float64 with pcl=True: PCL's own
    formulae -- the acos comparison, v scaled by 1 / |v|.  swap: force the swap choice (None: the rule's / PCL's)."""
    p, n_p, q, n_q = (np.asarray(a, dtype) for a in (p, n_p, q, n_q))
    with np.errstate(all="ignore"):
        dp = q - p
        f4 = np.sqrt(_dot(dp, dp))
        a1 = _dot(n_p, dp) / f4
        a2 = _dot(n_q, dp) / f4
        if swap is None:
            if pcl:
                swap = np.arccos(np.minimum(np.abs(a1), 1.0)) > np.arccos(np.minimum(np.abs(a2), 1.0))
            else:
                swap = np.abs(a1) < np.abs(a2)
        s = swap[..., None]
        n1 = np.where(s, n_q, n_p)
        n2 = np.where(s, n_p, n_q)
        dp = np.where(s, -dp, dp)
        f3 = np.where(swap, -a2, a1)
        v = _cross(dp, n1)
        vn = np.sqrt(_dot(v, v))
        v = v * (dtype(1.0) / vn)[..., None] if pcl else v / vn[..., None]
        w = _cross(n1, v)
        f2 = _dot(v, n2)
        f1 = np.arctan2(_dot(w, n2), _dot(n1, n2)).astype(dtype)
        pi, inv2pi = (dtype(np.pi), dtype(1.0 / (2.0 * np.pi))) if dtype is not F else (PI32, INV2PI32)
        x1 = (f1 + pi) * inv2pi
        x2 = (f2 + dtype(1.0)) * dtype(0.5)
        x3 = (f3 + dtype(1.0)) * dtype(0.5)
        zero_n = (np.all(n_p == 0, axis=-1)) | (np.all(n_q == 0, axis=-1))
        ok = (f4 != 0) & (vn != 0) & ~zero_n & np.isfinite(f4)
        bins = np.stack([_bin(x1, dtype), _bin(x2, dtype), _bin(x3, dtype)], axis=-1)
    bins = np.where(ok[..., None], bins, 0).astype(np.int32)
    return dict(ok=ok, swap=swap, a1=a1, a2=a2, f1=f1, f2=f2, f3=f3, x1=x1, x2=x2, x3=x3, bins=bins)


def _pairs(cloud, normals, idx, d2):
    """(p, n_p, q, n_q, live) of every list entry: [n, k, 3] x 4 and the entries the first pass looks at at all."""
    cloud = np.ascontiguousarray(cloud, F)[:, :3]
    nrm = np.ascontiguousarray(normals, F)[:, :3]
    n, k = idx.shape
    safe = np.where(idx >= 0, idx, 0)
    finite = np.isfinite(cloud).all(axis=1)
    live = (idx >= 0) & (d2 != 0) & finite[:, None]
    p = np.broadcast_to(cloud[:, None, :], (n, k, 3))
    n_p = np.broadcast_to(nrm[:, None, :], (n, k, 3))
    return p, n_p, cloud[safe], nrm[safe], live


def near_integer(x, eps=AMBIGUOUS_EPS):
    x = BINS * np.asarray(x, np.float64)
    return np.abs(x - np.round(x)) < eps


def spfh(cloud, normals, idx, d2):
    """The first pass -> (counts [n, 33] uint8, f1_risky [n] int: pairs of the point whose f1 bin coordinate, computed
    in float64, lies within 1e-4 of an integer -- atan2f is the one function of the rule that is not bit-defined)."""
    p, n_p, q, n_q, live = _pairs(cloud, normals, idx, d2)
    f = pair_features(p, n_p, q, n_q)
    ok = f["ok"] & live
    n = len(idx)
    counts = np.zeros((n, DIM), np.int32)
    rows = np.broadcast_to(np.arange(n)[:, None], ok.shape)
    for b in range(3):
        np.add.at(counts, (rows[ok], b * BINS + f["bins"][..., b][ok]), 1)
    f64 = pair_features(p, n_p, q, n_q, dtype=np.float64, swap=f["swap"])
    risky = (ok & near_integer(f64["x1"])).sum(axis=1)
    return counts.astype(np.uint8), risky


def weight(counts, idx, d2, cloud, normals):
    """The second pass on given counts and lists -> [n, 33] float32."""
    counts = np.asarray(counts)
    cloud = np.ascontiguousarray(cloud, F)[:, :3]
    nrm = np.ascontiguousarray(normals, F)[:, :3]
    n, k = idx.shape
    valid = np.isfinite(cloud).all(axis=1) & ~np.all(nrm == 0, axis=1)
    acc = np.zeros((n, DIM), F)
    with np.errstate(all="ignore"):
        for j in range(k):
            use = valid & (idx[:, j] >= 0) & (d2[:, j] != 0)
            w = F(1.0) / d2[:, j].astype(F)
            term = counts[np.where(idx[:, j] >= 0, idx[:, j], 0)].astype(F) * w[:, None]
            acc = np.where(use[:, None], acc + term, acc)
        out = np.zeros((n, DIM), F)
        for f in range(3):
            blk = acc[:, f * BINS:(f + 1) * BINS]
            s = blk[:, 0].copy()
            for b in range(1, BINS):
                s = s + blk[:, b]
            scale = np.where(s != 0, F(100.0) / s, F(0.0)).astype(F)
            out[:, f * BINS:(f + 1) * BINS] = blk * scale[:, None]
    out[~valid] = 0
    return out


def fpfh(cloud, normals, idx, d2):
    counts, risky = spfh(cloud, normals, idx, d2)
    return counts, weight(counts, idx, d2, cloud, normals), risky


def match(a, b, reciprocal=False):
    """-> (idx [na] int32, d2 [na] float32): the rule's match, a loop over the 33 bins vectorised over pairs."""
    a = np.ascontiguousarray(a, F)[:, :DIM]
    b = np.ascontiguousarray(b, F)[:, :DIM]

    def one(x, y):
        nx, ny = len(x), len(y)
        idx = np.full(nx, -1, np.int32)
        d2o = np.zeros(nx, F)
        y_ok = np.any(y != 0, axis=1) if ny else np.zeros(0, bool)
        if ny == 0 or not y_ok.any():
            return idx, d2o
        for s in range(0, nx, 1024):
            xs = x[s:s + 1024]
            d = np.zeros((len(xs), ny), F)
            for c in range(DIM):
                df = xs[:, c, None] - y[None, :, c]
                d = d + df * df
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(ny, dtype=np.uint64)[None, :]
            key[:, ~y_ok] = np.uint64(0xFFFFFFFFFFFFFFFF)
            best = key.min(axis=1)
            idx[s:s + 1024] = (best & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
            d2o[s:s + 1024] = (best >> np.uint64(32)).astype(np.uint32).view(F)
        zero = ~np.any(x != 0, axis=1)
        idx[zero] = -1
        d2o[zero] = 0
        return idx, d2o

    ia, da = one(a, b)
    if reciprocal and len(b):
        ib, _ = one(b, a)
        keep = (ia >= 0) & (ib[np.where(ia >= 0, ia, 0)] == np.arange(len(a)))
        ia = np.where(keep, ia, -1).astype(np.int32)
        da = np.where(keep, da, F(0)).astype(F)
    return ia, da


# ---- the clouds of the tests (built once)
_CLOUDS = {}


def clouds(n=6000):
    """name -> float32 [n, 3]: the two synthetic scenes in the sensor frame (z - 1.73: unshifted, their ground passes
    through the origin and the normal flip of 40 % of the points is noise) with 0.02 m of Gaussian noise, and n random
    points of the scan fixture."""
    if n not in _CLOUDS:
        import os
        from libwave_amd import pcd, synth
        out = {}
        for name, fn in (("scene", synth.scene), ("rings", synth.scene_rings)):
            c = np.asarray(fn(n, seed=5), np.float64)[:, :3]
            c[:, 2] -= 1.73
            c += np.random.default_rng(17).normal(0, 0.02, c.shape)
            out[name] = np.ascontiguousarray(c, F)
        scan = np.asarray(pcd.load_pcd_xyz(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testscan.pcd")), F)[:, :3]
        scan = scan[np.isfinite(scan).all(axis=1)]
        out["scan"] = np.ascontiguousarray(scan[np.random.default_rng(18).choice(len(scan), n, replace=False)])
        for v in out.values():
            v.setflags(write=False)
        _CLOUDS[n] = out
    return _CLOUDS[n]
