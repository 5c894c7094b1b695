"""The checker of the outlier filters, checked (tests/outlier_reference.py), and what of wm_outlier_filter and
wave::OutlierRemoval can be checked without a device.

  a. the checker against an independent computation: scipy's cKDTree in float64.
  b. the condition every comparison of tests/test_outlier_gpu.py rests on: on every (shape, mean_k) it runs, at its
     stddev_mult, no finite point lies within 4 float32 ulps of the threshold (the fence is empty) -- or every distance
     is one value, the variance exactly 0 and nothing removed -- and summing in another order moves the threshold by
     far less than a float ulp.  So the device's labels must equal the checker's, whatever order its sums take.
     Measured here: the fence is empty everywhere except `point` at every mean_k, `lattice` at mean_k = 1 and `dups` at
     mean_k = 1 (all distances 0, 0.5 and 0: dyadic, their sums exact in any order); the closest point elsewhere is 79
     float ulps from its threshold (exact_plane, mean_k 8); a plain reversed-order double sum moves a threshold by at
     most 2.2e-13 of its value (lattice, mean_k 8, where the variance is 1e-3 of the squared mean; 3.2e-14 elsewhere):
     a float ulp is 6e-8.  The 270 000-point scene at mean_k 8: the nearest point is 1.9e-7 (6.5 float ulps) from the
     threshold 0.2791, outside the fence of 4; the reversed sum moves that threshold by 4.7e-14.
  c. the C++ class: headers compile alone, YAML constructor, construction and copies without a device.
  d. wm_outlier_filter's argument checks, which come before a device is touched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import knn_reference as KR
import outlier_reference as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
YAML = os.path.join(ROOT, "tests", "golden", "config", "outlier_removal.yaml")
HEADERS = ["wave/matching/outlier_removal.hpp", "wave/matching/impl/outlier_removal.hpp"]
DEGENERATE = {("point", 1), ("point", 8), ("point", 31), ("lattice", 1), ("dups", 1)}  # one distance value, variance 0

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


# ------------------------------------------------------------------ a. against scipy in float64
@pytest.mark.parametrize("name", ["scene", "noisy_plane"])
def test_checker_agrees_with_a_float64_kdtree(name):
    from scipy.spatial import cKDTree
    cloud = KR.shapes()[name]
    c64 = cloud.astype(np.float64)
    tree = cKDTree(c64)
    for mean_k in OR.MEAN_KS:
        dd, _ = tree.query(c64, k=mean_k + 1)
        d64 = dd[:, 1:].mean(1)
        ref = OR.statistical(cloud, mean_k, OR.STDDEV_MULT)
        rel = np.abs(ref["dist"].astype(np.float64) - d64) / d64
        print("%s mean_k %d: max relative distance difference %.3e" % (name, mean_k, rel.max()))
        assert rel.max() <= 1e-6, (name, mean_k)
        n = len(d64)
        thr64 = d64.mean() + OR.STDDEV_MULT * np.sqrt((np.sum(d64 * d64) - d64.sum() ** 2 / n) / (n - 1))
        assert abs(thr64 - ref["threshold"]) <= 1e-6 * thr64
        clear = np.abs(d64 - thr64) > 1e-5 * thr64  # outside the float64 version's own fence
        assert clear.mean() > 0.99
        assert np.array_equal((d64 > thr64)[clear], (ref["labels"] == OR.OUTLIER)[clear]), (name, mean_k)


def test_radius_counts_agree_with_a_float64_kdtree():
    """the counts are equal wherever no pair lies within 1e-5 of the radius in float64"""
    from scipy.spatial import cKDTree
    cloud = KR.shapes()["scene"]
    c64 = cloud.astype(np.float64)
    tree = cKDTree(c64)
    for r in OR.RADII:
        inner = np.array([len(v) for v in tree.query_ball_point(c64, r * (1 - 1e-5))]) - 1
        outer = np.array([len(v) for v in tree.query_ball_point(c64, r * (1 + 1e-5))]) - 1
        counts, _ = OR.radius_counts(cloud, r)
        assert ((counts >= inner) & (counts <= outer)).all(), r
        assert (inner == outer).mean() > 0.99


def test_checker_on_cases_small_enough_to_read():
    c = np.float32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0], [1, 0, 0], [9, 0, 0]])
    ref = OR.statistical(c, 2, 0.0)
    # lists: 0: (0, 1, 1)  1: (0, 0 [its duplicate], 1)  3: (0, 4, 5)  4: as 1  5: (0, 64, 64)
    want = [(1 + 1) / 2, (0 + 1) / 2, 0, (2 + np.sqrt(5.0)) / 2, 0.5, 8.0]
    assert np.array_equal(ref["dist"], np.float32(want))
    assert ref["n_finite"] == 5 and ref["labels"].tolist() == [1, 1, 0, 1, 1, 2] and ref["kept"].tolist() == [0, 1, 3, 4]
    assert OR.statistical(c, 2, 0.0, negative=True)["kept"].tolist() == [5]
    rr = OR.radius(c, 1.0, 1)  # strict: the points at exactly 1 m are no neighbours; the duplicates are each other's
    assert rr["counts"].tolist() == [0, 1, -1, 0, 1, 0] and rr["kept"].tolist() == [1, 4]
    assert OR.radius(c, 1.0, 1, negative=True)["kept"].tolist() == [0, 3, 5]
    assert OR.radius(c, 1.0001, 2)["counts"].tolist() == [2, 2, -1, 0, 2, 0]
    assert OR.radius(c, 1.0, 0)["kept"].tolist() == [0, 1, 3, 4, 5]


# ------------------------------------------------------------------ b. the condition of the device comparison
def _condition(name, mean_k, ref):
    thr = ref["threshold"]
    shift = abs(ref["threshold_reversed"] - thr)
    print("%s mean_k %d: threshold %.9g, variance %.3g, fence %d, removed %d, reversed sum moves it by %.2e (float ulp %.2e)"
          % (name, mean_k, thr, ref["var"], len(ref["fence"]), (ref["labels"] == OR.OUTLIER).sum(), shift, OR.ulp32(thr)))
    if len(ref["fence"]):
        d = ref["dist"][ref["finite"]]
        assert ref["var"] == 0.0 and (d == d[0]).all() and not (ref["labels"] == OR.OUTLIER).any(), (name, mean_k)
        assert shift == 0.0
    assert shift < OR.ulp32(thr) or thr == 0.0, (name, mean_k)
    return shift / thr if thr else 0.0


@pytest.mark.parametrize("name", KR.NAMES)
def test_fence_is_empty_or_the_variance_exactly_zero(name):
    cloud = KR.shapes()[name]
    for mean_k in OR.MEAN_KS:
        ref = OR.statistical(cloud, mean_k, OR.STDDEV_MULT)
        rel = _condition(name, mean_k, ref)
        assert (len(ref["fence"]) > 0) == ((name, mean_k) in DEGENERATE), (name, mean_k)
        assert rel <= 1e-12
    if name == "clumps_outliers":
        far = np.nonzero(np.abs(cloud).max(1) > 20)[0]
        assert len(far) == 12
        for mean_k in OR.MEAN_KS:
            assert np.array_equal(np.nonzero(OR.statistical(cloud, mean_k, OR.STDDEV_MULT)["labels"] == OR.OUTLIER)[0], far)


def test_fence_is_empty_on_the_large_scene(oracle):
    cloud, ref = OR.big_case(oracle)
    _condition("scene(%d)" % len(cloud), OR.BIG_MEAN_K, ref)
    assert len(ref["fence"]) == 0
    gap = np.abs(ref["dist"].astype(np.float64) - ref["threshold"]).min()
    print("nearest point %.3e from the threshold = %.1f float ulps" % (gap, gap / OR.ulp32(ref["threshold"])))
    assert gap > OR.FENCE_ULPS * OR.ulp32(ref["threshold"])


def test_lattice_is_the_strict_comparison_case():
    cloud = KR.shapes()["lattice"]
    r2 = np.float32(0.25)
    d = cloud[:, None, :] - cloud[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert (d2 == r2).sum() == 18900  # (query, neighbour) pairs at exactly the radius: 3 axes x 14 x 15 x 15, both ways
    ref = OR.radius(cloud, 0.5, OR.MIN_NEIGHBORS)
    assert (ref["counts"] == 0).all() and len(ref["kept"]) == 0


# ------------------------------------------------------------------ c. the C++ class without a device
@needs_gxx
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_standalone(tmp_path, header):
    src = tmp_path / "one.cpp"
    src.write_text("#include <%s>\n" % header)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_yaml_and_construction_without_a_device(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "outlier_cpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_outlier", "outlier_cpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, YAML], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


# ------------------------------------------------------------------ d. the C ABI's argument checks
def _call(wm, ctx=C.c_void_p(1), n=10, stride=12, mem=None, out_mem=None, params="default", n_out="n_out", cap=10, idx="idx",
          pts="pts", **fields):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    cloud = np.zeros((10, 4), np.float32)
    out = np.zeros(16, np.int32)
    m = C.c_size_t(77)
    p = wm.outlier_params(dict(dict(method=wm.WM_OUTLIER_STATISTICAL, mean_k=8, stddev_mult=1.0, radius=0.5), **fields))
    return wm.lib().wm_outlier_filter(
        ctx, C.c_void_p(cloud.ctypes.data) if pts == "pts" else None, n, stride, wm.WM_MEM_HOST if mem is None else mem,
        C.byref(p) if params == "default" else None, C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap,
        wm.WM_MEM_HOST if out_mem is None else out_mem, C.byref(m) if n_out == "n_out" else None, None, None, None, None)


@pytest.mark.parametrize("bad", [dict(ctx=None), dict(params=None), dict(n_out=None), dict(stride=8), dict(stride=10),
                                 dict(stride=14), dict(mem=5), dict(out_mem=7), dict(method=2), dict(method=-1),
                                 dict(mean_k=0), dict(mean_k=32), dict(mean_k=50), dict(mean_k=-3), dict(pts=None),
                                 dict(idx=None), dict(n=0x7FFFFFF1),
                                 dict(method=1, radius=0.0), dict(method=1, radius=-1.0), dict(method=1, radius=float("nan")),
                                 dict(method=1, radius=float("inf")), dict(method=1, min_neighbors=-1)])
def test_argument_errors_without_a_device(wm, bad):
    assert _call(wm, **bad) == wm.WM_ERR_ARG


def test_empty_cloud_is_ok_without_a_device(wm):
    m = C.c_size_t(77)
    for method in (wm.WM_OUTLIER_STATISTICAL, wm.WM_OUTLIER_RADIUS):
        p = wm.outlier_params(method=method, mean_k=31, radius=1e-3, min_neighbors=0)
        st = wm.OutlierStats()
        st.n_finite = 9
        assert wm.lib().wm_outlier_filter(C.c_void_p(1), None, 0, 12, wm.WM_MEM_HOST, C.byref(p), None, 0, wm.WM_MEM_DEVICE,
                                          C.byref(m), None, None, None, C.byref(st)) == wm.WM_OK
        assert m.value == 0 and st.n_finite == 0


def test_symbols_defaults_and_the_python_surface(wm):
    assert {"wm_outlier_filter", "wm_outlier_default_params"} <= set(wm.declared_symbols())
    p = wm.outlier_params()  # PCL's defaults
    assert (p.method, p.mean_k, p.stddev_mult, p.radius, p.min_neighbors, p.negative) == (0, 1, 0.0, 0.0, 1, 0)
    assert (wm.WM_OUTLIER_NONE, wm.WM_OUTLIER_INLIER, wm.WM_OUTLIER_OUTLIER) == (OR.NONE, OR.INLIER, OR.OUTLIER)
    assert wm.WM_OUTLIER_MAX_MEAN_K == OR.MAX_MEAN_K == 31
    q = wm.outlier_params(dict(mean_k=8), radius=0.25)
    assert q.mean_k == 8 and q.radius == 0.25
    with pytest.raises(AttributeError):
        wm.outlier_params(leaf=1.0)
    assert hasattr(wm.Context, "outlier_filter")
    assert C.sizeof(wm.OutlierParams) == 32 and C.sizeof(wm.OutlierStats) == 56
