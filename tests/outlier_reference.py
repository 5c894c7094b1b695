"""The two outlier filters of wm_outlier_filter (libwave_amd/csrc/wm_outlier.hip) restated in float32 / float64 numpy:
the checker of tests/test_outlier_gpu.py, in the manner of knn_reference.py, on whose brute-force lists it stands.

  statistical  per finite point the mean_k + 1 nearest points by (float32 d2, index), itself included; entry 0 (d2 = 0:
               the point or a duplicate) skipped; s = sqrt((double) d2_j) added over entries 1 ... mean_k in list order in
               double; dist = (float) (s / mean_k).  Over the n finite points, dist widened to double: mean = sum d / n,
               var = (sum d^2 - (sum d)^2 / n) / (n - 1), stddev = sqrt(var), threshold = mean + stddev_mult * stddev;
               outlier iff (double) dist > threshold (a NaN threshold removes nothing).  The two sums are math.fsum's:
               the correctly rounded values, which no summation order of the device's can be told from by more than a
               few 1e-16 (threshold_reversed measures one such order).
  fence        the finite points with |dist - threshold| <= 4 float32 ulps of the threshold: the only points whose label
               could depend on how the sums were rounded.  tests/test_outlier_reference_cpu.py asserts that it is empty
               (or the variance exactly 0) wherever the device is compared, so the device's labels must EQUAL these.
  radius       r2 = (float32) (radius * radius), the product in double; count = the OTHER finite points with d2 < r2
               (strict), d2 formed as knn_reference forms it; inlier iff count >= min_neighbors.
  both         a non-finite point: label NONE, distance 0 / count -1, in neither the kept nor the removed list; kept
               indices ascend; negative returns the outliers."""
import math

import numpy as np

import knn_reference as KR

NONE, INLIER, OUTLIER = 0, 1, 2
MAX_MEAN_K = 31
FENCE_ULPS = 4


def mean_distances(cloud, mean_k, nbrs=None):
    """-> (dist [n] float32, 0 for a non-finite point; finite [n] bool).  nbrs: (idx, d2) lists of mean_k + 1 entries
    per point, ascending by (d2, index), the point itself first (KR.brute's by default)."""
    assert 1 <= mean_k <= MAX_MEAN_K
    cloud = np.ascontiguousarray(cloud, np.float32)
    finite = np.isfinite(cloud).all(1)
    assert finite.sum() >= mean_k + 1
    _, d2 = nbrs if nbrs is not None else KR.brute(cloud, mean_k + 1)
    assert d2.dtype == np.float32 and d2.shape == (len(cloud), mean_k + 1)
    s = np.zeros(len(cloud), np.float64)
    for j in range(1, mean_k + 1):  # list order
        s = s + np.sqrt(d2[:, j].astype(np.float64))
    dist = (s / np.float64(mean_k)).astype(np.float32)
    dist[~finite] = 0
    return dist, finite


def _threshold(s1, s2, n, stddev_mult):
    mean = s1 / n
    var = (s2 - s1 * s1 / n) / (n - 1) if n > 1 else float("nan")
    sd = math.sqrt(var) if var >= 0 else float("nan")
    return mean, var, sd, mean + stddev_mult * sd


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def statistical(cloud, mean_k, stddev_mult, negative=False, nbrs=None):
    dist, finite = mean_distances(cloud, mean_k, nbrs)
    d = dist[finite].astype(np.float64)
    n = len(d)
    mean, var, sd, thr = _threshold(math.fsum(d), math.fsum(d * d), n, stddev_mult)  # (d * d is exact in double)
    # one order a plain loop would take, for the CPU test's measurement of what the order is worth
    r1 = r2 = 0.0
    for v in d[::-1].tolist():
        r1 += v
        r2 += v * v
    thr_rev = _threshold(r1, r2, n, stddev_mult)[3]
    outlier = finite & (dist.astype(np.float64) > thr)  # (False everywhere for a NaN threshold)
    labels = np.where(finite, np.where(outlier, OUTLIER, INLIER), NONE).astype(np.uint8)
    fence = finite & (np.abs(dist.astype(np.float64) - thr) <= FENCE_ULPS * ulp32(thr)) if math.isfinite(thr) else np.zeros_like(finite)
    return dict(dist=dist, finite=finite, n_finite=n, mean=mean, var=var, stddev=sd, threshold=thr,
                threshold_reversed=thr_rev, labels=labels, fence=np.nonzero(fence)[0],
                kept=np.nonzero(labels == (OUTLIER if negative else INLIER))[0].astype(np.int32))


def radius_counts(cloud, radius, chunk=256):
    """-> (counts [n] int32, -1 for a non-finite point; finite [n] bool)"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    finite = np.isfinite(cloud).all(1)
    cand = np.nonzero(finite)[0]
    c = cloud[cand]
    r2 = np.float32(float(radius) * float(radius))
    counts = np.full(len(cloud), -1, np.int32)
    for s in range(0, len(cand), chunk):
        q = c[s:s + chunk]
        dx = q[:, None, 0] - c[None, :, 0]
        dy = q[:, None, 1] - c[None, :, 1]
        dz = q[:, None, 2] - c[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz  # float32 arrays: every operation rounded, none fused (as KR._top)
        assert d2.dtype == np.float32
        within = d2 < r2
        within[np.arange(len(q)), np.arange(s, s + len(q))] = False  # not the point itself
        counts[cand[s:s + chunk]] = within.sum(1)
    return counts, finite


def radius(cloud, radius_m, min_neighbors, negative=False):
    counts, finite = radius_counts(cloud, radius_m)
    outlier = finite & (counts < min_neighbors)
    labels = np.where(finite, np.where(outlier, OUTLIER, INLIER), NONE).astype(np.uint8)
    return dict(counts=counts, finite=finite, n_finite=int(finite.sum()), labels=labels,
                kept=np.nonzero(labels == (OUTLIER if negative else INLIER))[0].astype(np.int32))


# what tests/test_outlier_gpu.py runs, and tests/test_outlier_reference_cpu.py certifies the fence of
MEAN_KS = [1, 8, 31]
STDDEV_MULT = 1.0
RADII = [0.05, 0.5, 2.0]
MIN_NEIGHBORS = 5
BIG_N, BIG_SEED, BIG_MEAN_K = 270000, 5, 8  # one size above the 256k sort switch (synth.scene)

_BIG = None


def big_case(oracle):
    """-> (cloud, statistical(...)) of the large case, its lists from the oracle's kd-tree (a brute force over 270 000
    points is out of reach; tests/test_knn_reference_cpu.py holds the two to each other bit for bit).  Computed once."""
    global _BIG
    if _BIG is None:
        from libwave_amd import synth
        cloud = synth.scene(BIG_N, seed=BIG_SEED)
        assert np.isfinite(cloud).all()
        nbrs = oracle.KdTree(cloud).knn(cloud, BIG_MEAN_K + 1)
        _BIG = (cloud, statistical(cloud, BIG_MEAN_K, STDDEV_MULT, nbrs=nbrs))
    return _BIG
