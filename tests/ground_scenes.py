"""Small hand-made scenes for the ground filter (tests/test_ground_reference_cpu.py works their labels out by hand;
tests/test_ground_gpu.py runs them on the device against tests/ground_reference.py), and the larger workloads."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "config", "ground_segmentation.yaml")
SMALL = dict(rmax=10.0, num_bins_a=4, num_bins_l=10)  # 90-degree sectors, 1 m bins


def cell_points(deg, r, zs, jitter=0.0):
    """len(zs) points at azimuth `deg` (degrees) and ground range ~r (m), heights zs."""
    zs = np.asarray(zs, np.float64)
    k = np.arange(len(zs))
    a = math.radians(deg) + 0.002 * (k - len(zs) / 2.0)
    rr = r + jitter * (k - len(zs) / 2.0) + 0.01 * k
    return np.stack([rr * np.cos(a), rr * np.sin(a), zs], axis=1).astype(np.float32)


def disc(deg=45.0, bins=range(1, 9), per=6, z=0.0):
    """Flat ground: `per` points per 1 m bin at heights z + a few mm."""
    return np.concatenate([cell_points(deg, b + 0.5, z + 0.002 * np.arange(per)) for b in bins])


def with_params(**kw):
    p = dict(SMALL)
    p.update(kw)
    return p


def rings_sensor_frame(n, seed=42):
    """synth.scene_rings shifted to the sensor frame (z - 1.73): the lidar at the origin, the ground at -1.73."""
    from libwave_amd import synth
    pts = synth.scene_rings(n, seed=seed)
    pts[:, 2] -= np.float32(1.73)
    return np.ascontiguousarray(pts)


def large_model(n=200_000, seed=5):
    """num_bins_a = 8, num_bins_l = 400 (0.25 m bins to 100 m): a dense, gently sloped plane with walls and boxes on
    it -- every sector's ground model grows well above 200 cells."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = int(0.85 * n)
    r = rng.uniform(0.3, 99.5, m)
    a = rng.uniform(0.0, 2 * np.pi, m)
    x, y = r * np.cos(a), r * np.sin(a)
    z = -1.73 + 0.004 * x + 0.002 * y + rng.normal(0.0, 0.01, m)
    ground = np.stack([x, y, z], axis=1)
    k = n - m
    cx = rng.uniform(-60, 60, 40)
    cy = rng.uniform(-60, 60, 40)
    w = rng.integers(0, 40, k)
    bx = cx[w] + rng.uniform(-1.0, 1.0, k)
    by = cy[w] + rng.uniform(-1.0, 1.0, k)
    bz = -1.73 + 0.004 * bx + 0.002 * by + rng.uniform(0.2, 3.5, k)
    pts = np.concatenate([ground, np.stack([bx, by, bz], axis=1)])
    pts = pts[rng.permutation(len(pts))]
    return np.ascontiguousarray(pts, dtype=np.float32)
