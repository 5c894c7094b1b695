"""The k nearest neighbours of every point of a cloud in the cloud itself, by brute force in float32 numpy: the checker of
knn_search<K> (libwave_amd/csrc/wm_gicp_dev.hpp), in the manner of plane_reference.py / info_reference.py.

  brute    every pair's squared distance formed as g_d2 forms it -- d2 = (dx * dx + dy * dy) + dz * dz, each operation
           rounded to float32, nothing fused -- and the k smallest 64-bit keys (bits of d2) << 32 | caller index per
           query, ascending: the order the kernels claim (distance, then index).  A non-finite point is no neighbour of
           anything; its own row is -1 / 0, as are the places of a list that the cloud is too small to fill.
  shapes   the stress clouds: collapsed grid axes, duplicates, long runs and far outliers (the box grows many times),
           exact float ties straddling the k-th place, large offsets, non-finite points.  Float32, fixed seeds, at most
           ~3 400 points, so that a brute force costs a fraction of a second.

tests/test_knn_reference_cpu.py holds brute to the oracle's kd-tree on every shape; tests/test_knn_stress_gpu.py holds
the device to brute."""
import numpy as np

from libwave_amd import synth

K_MAX = 33  # the longest list anything asks for: k = 32 and the neighbour after it (plane_reference.normals' tie test)
UTM = np.array([12345.0, -54321.0, 250.0])  # integers: subtracting them from float32 coordinates is exact in float64

_TOP = {}


def _top(cloud, chunk=256):
    """-> (keys [n, m] uint64 ascending, m = min(K_MAX, finite points); finite [n]): computed once per cloud."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    tag = (cloud.shape, cloud.tobytes())
    if tag in _TOP:
        return _TOP[tag]
    n = len(cloud)
    finite = np.isfinite(cloud).all(1)
    cand = np.nonzero(finite)[0]
    c = cloud[cand]
    m = min(K_MAX, len(cand))
    keys = np.full((n, m), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    for s in range(0, len(cand), chunk):
        q = c[s:s + chunk]
        dx = q[:, None, 0] - c[None, :, 0]
        dy = q[:, None, 1] - c[None, :, 1]
        dz = q[:, None, 2] - c[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz  # float32 arrays: numpy rounds every operation and fuses none
        assert d2.dtype == np.float32
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand[None, :].astype(np.uint64)
        part = np.partition(key, m - 1, axis=1)[:, :m] if m < key.shape[1] else key
        keys[cand[s:s + chunk]] = np.sort(part, axis=1)
    if len(_TOP) >= 16:
        _TOP.clear()
    _TOP[tag] = (keys, finite)
    return keys, finite


def brute(cloud, k):
    """-> (idx [n, k] int32, d2 [n, k] float32): the exact k nearest neighbours of every point (itself included),
    ascending by (float32 d2, index); -1 / 0 in a non-finite point's row and where fewer than k finite points exist."""
    assert 1 <= k <= K_MAX
    keys, finite = _top(cloud)
    n, m = keys.shape
    idx = np.full((n, k), -1, np.int32)
    d2 = np.zeros((n, k), np.float32)
    j = min(k, m)
    rows = np.nonzero(finite)[0]
    idx[rows, :j] = (keys[rows, :j] & np.uint64(0xFFFFFFFF)).astype(np.int32)
    d2[rows, :j] = (keys[rows, :j] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _noisy_plane():
    rng = np.random.default_rng(102)
    return np.c_[rng.uniform(-10, 10, (3000, 2)), rng.normal(0, 0.01, 3000) + 1.25]


def _build_shapes():
    out = {}
    rng = np.random.default_rng(101)
    out["exact_plane"] = _f32(np.c_[rng.uniform(-10, 10, (3000, 2)), np.full(3000, 1.25)])  # one grid axis collapses
    out["noisy_plane"] = _f32(_noisy_plane())
    rng = np.random.default_rng(103)
    out["line"] = _f32(np.c_[rng.uniform(-20, 20, 3000), np.full(3000, -3.0), np.full(3000, 0.5)])  # two axes collapse
    out["point"] = _f32(np.tile([[1.0, 2.0, 3.0]], (500, 1)))
    # long runs in two dense clumps, a huge bounding box, isolated queries whose box grows many times
    rng = np.random.default_rng(104)
    flat = np.array([1.0, 1.0, 0.05])
    a = rng.normal(0, 0.02, (1500, 3)) * flat + [5.0, 5.0, 0.0]
    b = rng.normal(0, 0.02, (1500, 3)) * flat[[2, 0, 1]] - [5.0, 5.0, 0.0]
    out["clumps_outliers"] = _f32(np.r_[a, b, rng.uniform(-300, 300, (12, 3))][rng.permutation(3012)])
    rng = np.random.default_rng(105)
    v = rng.normal(size=(3000, 3))
    out["shell"] = _f32(8.0 * v / np.linalg.norm(v, axis=1, keepdims=True))
    # 6-, 12- and 8-way exact float ties straddling the k-th place for most k; indices unrelated to position
    rng = np.random.default_rng(106)
    g = np.arange(-7, 8, dtype=np.float32) * np.float32(0.5)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out["lattice"] = _f32(lat[rng.permutation(len(lat))])
    rng = np.random.default_rng(107)
    base = rng.uniform(-5, 5, (1000, 3)).astype(np.float32)
    out["dups"] = _f32(np.r_[base, base[::-1], base])  # every point three times
    rng = np.random.default_rng(108)
    out["utm"] = _f32(rng.uniform(-15, 15, (3000, 3)) + UTM)  # ~1 mm float spacing in x, 4 mm in y
    out["utm_plane"] = _f32(_noisy_plane() + UTM)
    out["scene"] = synth.scene(3000, seed=5)
    holes = out["scene"].copy()
    holes[0] = np.nan
    holes[17, 1] = np.inf
    holes[1500, 2] = -np.inf
    holes[-1, 0] = np.nan
    out["holes"] = holes
    for c in out.values():
        c.setflags(write=False)
    return out


_SHAPES = None


def shapes():
    """name -> float32 [n, 3] (read-only, built once)."""
    global _SHAPES
    if _SHAPES is None:
        _SHAPES = _build_shapes()
    return _SHAPES


NAMES = ["exact_plane", "noisy_plane", "line", "point", "clumps_outliers", "shell", "lattice", "dups", "utm", "utm_plane",
         "scene", "holes"]
# the normals comparison (tests/test_knn_stress_gpu.py) and the cap on what it may leave out (1 %: the reference alone
# leaves out 0.1 % at the most on these; asserted on the CPU by tests/test_knn_reference_cpu.py)
NORMAL_SHAPES = ["noisy_plane", "exact_plane", "shell", "scene", "clumps_outliers", "utm_plane"]
NORMAL_KS = [8, 10, 12, 16, 24, 32]
NORMAL_CAP = 0.01


def normal_origin(name):
    """what plane_reference.normals subtracts (in float64, exactly) before it forms a covariance"""
    return UTM if name.startswith("utm") else None
