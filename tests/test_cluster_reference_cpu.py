"""The checker of the cluster extraction, checked (tests/cluster_reference.py), and what of wm_cluster_extract and
wave::EuclideanClusterExtraction can be checked without a device.

  a. the two forms of the checker against each other -- every pair by brute force against the kd-tree's candidate
     pairs -- on every (shape, tolerance) tests/test_cluster_gpu.py compares the device on.
  b. the inputs discriminate: the component counts and sizes that make a wrong strict test, a missed edge of a long
     path, a lost union on a contended root or a wrong size rule visible, asserted from the brute force.
  c. the C++ class: headers compile alone, YAML constructor, construction and copies without a device.
  d. wm_cluster_extract's argument checks, which come before a device is touched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cluster_reference as CR
import knn_reference as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
YAML = os.path.join(ROOT, "tests", "golden", "config", "cluster_extraction.yaml")
HEADERS = ["wave/matching/cluster_extraction.hpp", "wave/matching/impl/cluster_extraction.hpp",
           "wave/compat/pcl_indices_min.hpp"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _top(ref, k=4):
    s = ref["component_sizes"]
    return int(ref["n_components"]), s[:k].tolist(), int((s == 1).sum())


# ------------------------------------------------------------------ a. the two forms against each other
@pytest.mark.parametrize("name", KR.NAMES + sorted(CR.OWN))
def test_kdtree_form_equals_brute_force(name):
    cloud = CR.shapes()[name]
    for tol in [t for n, t in CR.CASES if n == name]:
        b, k = CR.brute_case(name, tol), CR.components(cloud, tol)
        print("%s %.9g: %d components, largest %s, %d singletons; %d edges, %d pairs at exactly r2"
              % ((name, tol) + _top(b) + (b["n_edges"], b["n_at_r2"])))
        for key in ("labels", "indices", "offsets"):
            assert np.array_equal(b[key], k[key]) and b[key].dtype == k[key].dtype, (name, tol, key)
        for key in ("n_clusters", "n_out", "n_finite", "n_components", "n_clustered", "largest", "n_edges"):
            assert b[key] == k[key], (name, tol, key)


def test_checker_on_a_case_small_enough_to_read():
    c = np.float32([[0, 0, 0], [5, 0, 0], [np.nan, 0, 0], [0.5, 0, 0], [5, 0.5, 0], [9, 0, 0], [1.0, 0, 0], [0, np.inf, 0]])
    ref = CR.components_brute(c, 0.6)
    # {0, 3, 6} (a chain), {1, 4}, {5}; 2 and 7 are non-finite
    assert ref["labels"].tolist() == [0, 1, -1, 0, 1, 2, 0, -1]
    assert ref["indices"].tolist() == [0, 3, 6, 1, 4, 5] and ref["offsets"].tolist() == [0, 3, 5, 6]
    assert (ref["n_finite"], ref["n_components"], ref["n_clusters"], ref["n_clustered"], ref["largest"]) == (6, 3, 3, 6, 3)
    strict = CR.components_brute(c, 0.5)  # the pairs at exactly 0.5 m are no neighbours
    assert strict["n_components"] == 6 and strict["n_at_r2"] == 3 and strict["labels"].tolist() == [0, 1, -1, 2, 3, 4, 5, -1]
    two = CR.components_brute(c, 0.6, min_cluster_size=2)
    assert two["labels"].tolist() == [0, 1, -1, 0, 1, -2, 0, -1] and two["offsets"].tolist() == [0, 3, 5]
    assert CR.components_brute(c, 0.6, 2, 2)["labels"].tolist() == [-2, 0, -1, -2, 0, -2, -2, -1]
    none = CR.components_brute(c, 0.6, 3, 2)  # max < min keeps nothing
    assert none["n_clusters"] == 0 and none["offsets"].tolist() == [0] and len(none["indices"]) == 0 and none["largest"] == 0
    assert CR.components_brute(c, 0.6, 0)["labels"].tolist() == ref["labels"].tolist()  # 0 acts as 1
    # equal sizes: by the smallest member index
    tie = CR.components_brute(np.float32([[9, 0, 0], [0, 0, 0], [9.1, 0, 0], [0.1, 0, 0]]), 0.2)
    assert tie["labels"].tolist() == [0, 1, 0, 1] and tie["indices"].tolist() == [0, 2, 1, 3]
    for key in ("labels", "indices", "offsets"):
        assert np.array_equal(CR.with_size_rule(ref, 2, 2)[key], CR.components_brute(c, 0.6, 2, 2)[key])


# ------------------------------------------------------------------ b. the inputs discriminate
def test_the_inputs_discriminate():
    B = CR.brute_case
    lat = B("lattice", 0.5)
    assert _top(lat)[0] == 3375 and _top(lat)[2] == 3375 and lat["n_at_r2"] == 9450  # the strict test: every pair AT r2
    assert _top(B("lattice", 0.5000001))[:2] == (1, [3375])
    rails = B("rails", 0.25)
    assert _top(rails)[:2] == (2, [1024, 1024]) and rails["n_at_r2"] == 1024 + 2044  # cross pairs, two-apart pairs
    assert _top(B("rails", 0.2500001))[0] == 1
    assert _top(B("rails", 0.125)) == (2048, [1, 1, 1, 1], 2048) and B("rails", 0.125)["n_at_r2"] == 2046
    assert _top(B("rails", 0.1250001))[:2] == (2, [1024, 1024])
    helix = B("helix", 0.1)
    assert _top(helix)[:2] == (1, [4096]) and helix["n_edges"] == 4095  # a path: every edge a bridge
    assert _top(B("helix", 0.08)) == (4096, [1, 1, 1, 1], 4096)
    for tol in CR.TOLERANCES:
        p = B("point", tol)
        assert _top(p)[:2] == (1, [500]) and p["n_edges"] == 124750  # every edge onto one root
        assert _top(B("clumps_outliers", tol)) == (14, [1500, 1500, 1, 1], 12)
    assert _top(B("dups", 0.05)) == (1000, [3, 3, 3, 3], 0)
    assert _top(B("line", 0.05)) == (81, [169, 139, 135, 113], 1) and _top(B("line", 0.5))[0] == 1
    assert _top(B("exact_plane", 0.5))[:2] == (15, [2972, 4, 4, 3])
    assert _top(B("noisy_plane", 0.5))[:2] == (29, [2915, 17, 14, 8])
    assert _top(B("utm_plane", 0.5))[:2] == (29, [2915, 17, 14, 8])
    assert _top(B("shell", 0.5)) == (473, [57, 55, 55, 54], 154)
    assert _top(B("utm", 2.0))[:2] == (210, [2308, 100, 52, 35])
    assert _top(B("scene", 2.0)) == (216, [446, 281, 170, 158], 82)
    holes = B("holes", 2.0)
    assert _top(holes)[0] == 216 and holes["largest"] == 445 and holes["n_finite"] == 2996
    assert (holes["labels"][[0, 17, 1500, 2999]] == CR.NONE).all() and not np.isin([0, 17, 1500, 2999], holes["indices"]).any()


def test_the_large_scene_discriminates():
    assert _top(CR.big_case(0.1)) == (162250, [496, 435, 422, 379], 111756)  # the ranking sort at size
    assert _top(CR.big_case(0.3))[:2] == (1495, [264439, 151, 115, 96])      # the union-find at size


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
    exe = str(tmp_path / "cluster_cpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_cluster", "cluster_cpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, YAML], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


# ------------------------------------------------------------------ d. the C ABI's argument checks
def _call(wm, ctx=C.c_void_p(1), n=10, stride=12, mem=None, out_mem=None, params="default", n_out="n_out",
          n_clusters="n_clusters", cap=10, cap_clusters=10, idx="idx", off="off", pts="pts", **fields):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    cloud = np.zeros((10, 4), np.float32)
    out = np.zeros(16, np.int32)
    offs = np.zeros(16, np.uint32)
    m, k = C.c_size_t(77), C.c_size_t(77)
    p = wm.cluster_params(dict(dict(tolerance=0.5), **fields))
    return wm.lib().wm_cluster_extract(
        ctx, C.c_void_p(cloud.ctypes.data) if pts == "pts" else None, n, stride, wm.WM_MEM_HOST if mem is None else mem,
        C.byref(p) if params == "default" else None, None, C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap,
        C.c_void_p(offs.ctypes.data) if off == "off" else None, cap_clusters, wm.WM_MEM_HOST if out_mem is None else out_mem,
        C.byref(k) if n_clusters == "n_clusters" else None, C.byref(m) if n_out == "n_out" else None, None)


@pytest.mark.parametrize("bad", [dict(ctx=None), dict(params=None), dict(n_out=None), dict(n_clusters=None), dict(stride=8),
                                 dict(stride=10), dict(stride=14), dict(mem=5), dict(out_mem=7), dict(pts=None),
                                 dict(idx=None), dict(off=None), dict(n=0x7FFFFFF1), dict(tolerance=0.0),
                                 dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=float("inf")),
                                 dict(min_cluster_size=-1), dict(max_cluster_size=-1)])
def test_argument_errors_without_a_device(wm, bad):
    assert _call(wm, **bad) == wm.WM_ERR_ARG


def test_empty_cloud_is_ok_without_a_device(wm):
    m, k = C.c_size_t(77), C.c_size_t(77)
    p = wm.cluster_params(tolerance=1e-3, min_cluster_size=0, max_cluster_size=0)
    st = wm.ClusterStats()
    st.n_finite = st.n_components = 9
    offs = np.full(1, 5, np.uint32)
    assert wm.lib().wm_cluster_extract(C.c_void_p(1), None, 0, 12, wm.WM_MEM_HOST, C.byref(p), None, None, 0,
                                       C.c_void_p(offs.ctypes.data), 0, wm.WM_MEM_HOST, C.byref(k), C.byref(m),
                                       C.byref(st)) == wm.WM_OK
    assert (m.value, k.value, st.n_finite, st.n_components, offs[0]) == (0, 0, 0, 0, 0)
    # device outputs: still no device touched (nothing can be written)
    assert wm.lib().wm_cluster_extract(C.c_void_p(1), None, 0, 16, wm.WM_MEM_DEVICE, C.byref(p), None, None, 0, None, 0,
                                       wm.WM_MEM_DEVICE, C.byref(k), C.byref(m), None) == wm.WM_OK


def test_symbols_defaults_and_the_python_surface(wm):
    assert {"wm_cluster_extract", "wm_cluster_default_params"} <= set(wm.declared_symbols())
    p = wm.cluster_params()  # PCL's defaults
    assert (p.tolerance, p.min_cluster_size, p.max_cluster_size) == (0.0, 1, 2 ** 31 - 1)
    assert (wm.WM_CLUSTER_NONE, wm.WM_CLUSTER_REJECTED) == (CR.NONE, CR.REJECTED) == (-1, -2)
    q = wm.cluster_params(dict(min_cluster_size=8), tolerance=0.25)
    assert q.min_cluster_size == 8 and q.tolerance == 0.25
    with pytest.raises(AttributeError):
        wm.cluster_params(radius=1.0)
    assert hasattr(wm.Context, "cluster_extract")
    assert C.sizeof(wm.ClusterParams) == 16 and C.sizeof(wm.ClusterStats) == 48
    import re
    hdr = open(os.path.join(ROOT, "include", "wavematch.h")).read()
    assert re.search(r"WM_CLUSTER_NONE = -1", hdr) and re.search(r"WM_CLUSTER_REJECTED = -2", hdr)


def test_the_option_is_in_the_table(wm):
    """cluster_cell_div has its row in the options table and in INTEGRATION.md's knob table"""
    src = open(os.path.join(ROOT, "libwave_amd", "csrc", "wm_ctx.hip")).read()
    assert '{"cluster_cell_div", "WM_TUNE_CLUSTER_CELL_DIV", nullptr, &wm_ctx::tune_cluster_cell_div, 0.5, 8, 0}' in src
    assert "`cluster_cell_div` | `WM_TUNE_CLUSTER_CELL_DIV` | 2 |" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
