"""The checker of the conditional cluster extraction, checked (tests/cluster_cond_reference.py), and what of
wm_cluster_extract_cond can be checked without a device.

  a. the two forms of the checker against each other on every case tests/test_cluster_cond_gpu.py compares the device
     on: the table's shapes, cluster_reference.CASES under the four conditions (with attributes from a float64 PCA in
     place of the device's normals: the forms must agree whatever the attributes are), the large scene.
  b. the table of component counts, from the all-pairs form.
  c. the bindings, the struct sizes, the header's text.
  d. wm_cluster_extract_cond's argument checks, which come before a device is touched."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cluster_cond_reference as CC
import cluster_reference as CR
import knn_reference as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("labels", "indices", "offsets")
COUNTS = ("n_clusters", "n_out", "n_finite", "n_components", "n_clustered", "largest", "n_edges", "n_near")


def _same(b, k, what):
    for key in KEYS:
        assert np.array_equal(b[key], k[key]) and b[key].dtype == k[key].dtype, (what, key)
    for key in COUNTS:
        assert b[key] == k[key], (what, key, b[key], k[key])


# ------------------------------------------------------------------ a. the two forms against each other
@pytest.mark.parametrize("name", KR.NAMES + sorted(CR.OWN))
def test_kdtree_form_equals_brute_force(name):
    cloud = CR.shapes()[name]
    attr = CC.pca_attributes(cloud)
    for tol in [t for n, t in CR.CASES if n == name]:
        kd = CC._kd_edges(cloud, tol)
        for angle, diff in CC.CONDITIONS:
            b = CC.brute_case(name, tol, attr, angle, diff)
            k = CC._restrict(len(cloud), kd, attr, angle, diff, 1, CC.INT_MAX)
            print("%s %.9g angle %s diff %s: %d components, %d of %d near pairs are edges"
                  % (name, tol, angle, diff, b["n_components"], b["n_edges"], b["n_near"]))
            _same(b, k, (name, tol, angle, diff))
            plain = CR.brute_case(name, tol)
            assert b["n_near"] == plain["n_edges"] and b["n_components"] >= plain["n_components"]


def test_kdtree_form_equals_brute_force_on_the_table():
    for what, (cloud, attr), tol, angle, diff, _, _ in CC.table():
        _same(CC.components_brute(cloud, attr, tol, angle, diff), CC.components(cloud, attr, tol, angle, diff), what)


def test_no_condition_is_the_unconditional_checker():
    for name, tol in (("scene", 2.0), ("holes", 2.0), ("rails", 0.25)):
        cloud = CR.shapes()[name]
        got = CC.components_brute(cloud, np.full((len(cloud), 4), np.nan, np.float32), tol)
        for key in KEYS:
            assert np.array_equal(got[key], CR.brute_case(name, tol)[key])


# ------------------------------------------------------------------ b. the table
def test_the_table_of_component_counts():
    for what, (cloud, attr), tol, angle, diff, n_comp, largest in CC.table():
        ref = CC.components_brute(cloud, attr, tol, angle, diff)
        assert ref["n_components"] == n_comp, (what, ref["n_components"])
        assert ref["component_sizes"][:len(largest)].tolist() == largest, what
        assert ref["n_finite"] == len(cloud) and (ref["labels"] >= 0).all(), what
    (cloud, attr) = CC.triple(middle_s=np.nan)
    assert CC.components_brute(cloud, attr, 0.2, None, 5.0)["labels"].tolist() == [0, 1, 0]
    (cloud, attr) = CC.triple(middle_normal=(0.0, 0.0, 0.0))
    assert CC.components_brute(cloud, attr, 0.2, 30 * CC.DEG, None)["labels"].tolist() == [0, 1, 0]
    assert CC.cos_min(math.pi / 2) > 0
    # min_cluster_size cuts the fan's singletons
    cloud, attr = CC.shapes()["fan"]
    cut = CC.components_brute(cloud, attr, 0.2, 4 * CC.DEG, None, min_cluster_size=2)
    assert cut["n_clusters"] == 0 and (cut["labels"] == CC.REJECTED).all() and cut["n_components"] == 64


# ------------------------------------------------------------------ c. the surface
def test_symbols_sizes_and_the_python_surface(wm):
    assert {"wm_cluster_extract_cond", "wm_cluster_cond_default"} <= set(wm.declared_symbols())
    assert C.sizeof(wm.ClusterCond) == 24 and C.sizeof(wm.ClusterParams) == 16 and C.sizeof(wm.ClusterStats) == 48
    assert (wm.WM_CLUSTER_COND_NORMAL, wm.WM_CLUSTER_COND_SCALAR) == (1, 2)
    c = wm.ClusterCond(3, 7, 1.0, 2.0)
    wm.lib().wm_cluster_cond_default(C.byref(c))
    assert (c.flags, c.reserved, c.max_normal_angle, c.max_scalar_diff) == (0, 0, 0.0, 0.0)
    wm.lib().wm_cluster_cond_default(None)
    c = wm.cluster_cond(max_normal_angle=0.5)
    assert (c.flags, c.max_normal_angle, c.max_scalar_diff) == (1, 0.5, 0.0)
    c = wm.cluster_cond(dict(flags=2, max_scalar_diff=0.25), max_normal_angle=0.1)
    assert (c.flags, c.max_normal_angle, c.max_scalar_diff) == (3, 0.1, 0.25)
    assert wm.cluster_cond(c, flags=0).flags == 0 and wm.cluster_cond().flags == 0
    with pytest.raises(AttributeError):
        wm.cluster_cond(angle=1.0)
    assert hasattr(wm.Context, "cluster_extract_cond")
    import re
    hdr = open(os.path.join(ROOT, "include", "wavematch.h")).read()
    assert re.search(r"WM_CLUSTER_COND_NORMAL = 1, WM_CLUSTER_COND_SCALAR = 2", hdr)
    assert "6.1e-17" in hdr and "getRemovedClusters" in hdr and "[PCL-upstream" in hdr


# ------------------------------------------------------------------ d. the C ABI's argument checks
def _call(wm, ctx=C.c_void_p(1), n=10, stride=12, mem=None, out_mem=None, params="default", cond="default", n_out="n_out",
          n_clusters="n_clusters", cap=10, cap_clusters=10, idx="idx", off="off", pts="pts", attr="attr", attr_stride=16,
          attr_mem=None, flags=3, reserved=0, max_normal_angle=0.5, max_scalar_diff=0.5, **fields):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    cloud = np.zeros((10, 4), np.float32)
    at = np.zeros((10, 8), np.float32)
    out = np.zeros(16, np.int32)
    offs = np.zeros(16, np.uint32)
    m, k = C.c_size_t(77), C.c_size_t(77)
    p = wm.cluster_params(dict(dict(tolerance=0.5), **fields))
    c = wm.ClusterCond(flags, reserved, max_normal_angle, max_scalar_diff)
    return wm.lib().wm_cluster_extract_cond(
        ctx, C.c_void_p(cloud.ctypes.data) if pts == "pts" else None, n, stride, wm.WM_MEM_HOST if mem is None else mem,
        C.c_void_p(at.ctypes.data) if attr == "attr" else None, attr_stride, wm.WM_MEM_HOST if attr_mem is None else attr_mem,
        C.byref(p) if params == "default" else None, C.byref(c) if cond == "default" else None, None,
        C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap, C.c_void_p(offs.ctypes.data) if off == "off" else None,
        cap_clusters, wm.WM_MEM_HOST if out_mem is None else out_mem, C.byref(k) if n_clusters == "n_clusters" else None,
        C.byref(m) if n_out == "n_out" else None, None)


OWN = [dict(ctx=None), dict(params=None), dict(n_out=None), dict(n_clusters=None), dict(stride=8), dict(stride=10),
       dict(stride=14), dict(mem=5), dict(out_mem=7), dict(pts=None), dict(idx=None), dict(off=None), dict(n=0x7FFFFFF1),
       dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=float("inf")),
       dict(min_cluster_size=-1), dict(max_cluster_size=-1)]  # wm_cluster_extract's own
NEW = [dict(cond=None), dict(flags=4), dict(flags=-1), dict(flags=8), dict(reserved=1), dict(attr=None), dict(attr=None, flags=1),
       dict(attr=None, flags=2), dict(attr_stride=12), dict(attr_stride=18), dict(attr_stride=0), dict(attr_mem=2),
       dict(attr_mem=-1), dict(attr_stride=12, flags=0), dict(attr_mem=3, flags=0),
       dict(max_normal_angle=float("nan")), dict(max_normal_angle=float("inf")), dict(max_normal_angle=-1e-9),
       dict(max_normal_angle=math.nextafter(math.pi / 2, 4.0)), dict(max_normal_angle=2.0, flags=1),
       dict(max_scalar_diff=float("nan")), dict(max_scalar_diff=float("inf")), dict(max_scalar_diff=-1e-300),
       dict(max_scalar_diff=-1.0, flags=2)]


@pytest.mark.parametrize("bad", OWN + NEW)
def test_argument_errors_without_a_device(wm, bad):
    assert _call(wm, **bad) == wm.WM_ERR_ARG


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_empty_cloud_is_ok_without_a_device(wm, flags):
    """n == 0: WM_OK with no device touched, whatever the flags; a field its flag does not enable is not read"""
    assert _call(wm, n=0, pts=None, attr=None, idx=None, cap=0, flags=flags) == wm.WM_OK
    assert _call(wm, n=0, flags=0, attr=None, max_normal_angle=float("nan"), max_scalar_diff=-1.0) == wm.WM_OK
    assert _call(wm, n=0, flags=1, max_normal_angle=math.pi / 2, max_scalar_diff=-1.0) == wm.WM_OK
    assert _call(wm, n=0, flags=2, max_normal_angle=9.0, max_scalar_diff=0.0) == wm.WM_OK
    m, k = C.c_size_t(77), C.c_size_t(77)
    p, c = wm.cluster_params(tolerance=1e-3), wm.cluster_cond(flags=flags)
    st = wm.ClusterStats()
    st.n_finite = st.n_components = 9
    offs = np.full(1, 5, np.uint32)
    assert wm.lib().wm_cluster_extract_cond(C.c_void_p(1), None, 0, 12, wm.WM_MEM_HOST, None, 16, wm.WM_MEM_HOST, C.byref(p),
                                            C.byref(c), None, None, 0, C.c_void_p(offs.ctypes.data), 0, wm.WM_MEM_HOST,
                                            C.byref(k), C.byref(m), C.byref(st)) == wm.WM_OK
    assert (m.value, k.value, st.n_finite, st.n_components, offs[0]) == (0, 0, 0, 0, 0)
