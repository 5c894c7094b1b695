"""wm_cluster_extract_batch and EuclideanClusterExtraction<PointT>::extractBatch without a device: the symbol is
exported, the argument errors are found before a device is touched, the header still compiles on its own and a
translation unit that calls extractBatch on pcl::PointXYZ and on a 32-byte point type links against
libwave_matching.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_cluster_batch_cpp import ROOT, build_exe


def test_symbol_is_exported_and_declared(wm):
    assert "wm_cluster_extract_batch" in wm.declared_symbols()
    assert hasattr(wm.lib(), "wm_cluster_extract_batch")
    assert wm.WM_CLUSTER_BATCH_MAX_POINTS == 0x7FFFFFF0 and wm.WM_CLUSTER_BATCH_KEY_BITS == 64
    assert C.sizeof(wm.ClusterScan) == 16


def call(wm, ctx=C.c_void_p(1), n_scans=2, stride=12, mem=None, params=None, scans="table", first="first", n_out="n_out",
         n=10, sizes=None, null_pts=False, cap=10, idx="idx", cap_clusters=10, off="off", pts_out=None, out_stride=0,
         out_mem=None, p="p"):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    pts = np.zeros((4, 3), np.float32)  # (never read: every case here fails before, or touches nothing)
    S = max(n_scans, 0)
    rows = min(S, 5000)  # (a count beyond the limit is refused before the table is read)
    tab = (wm.ClusterScan * max(rows, 1))()
    for k in range(rows):
        tab[k].pts = None if null_pts else pts.ctypes.data
        tab[k].n = sizes[k] if sizes else n
    out = np.zeros(16, np.int32)
    offs = np.zeros(16, np.uint32)
    f = (C.c_size_t * (rows + 1))()
    m = C.c_size_t(0)
    par = wm.cluster_params(dict(dict(tolerance=0.5), **(params or {})))
    return wm.lib().wm_cluster_extract_batch(
        ctx, tab if scans == "table" else None, n_scans, stride, wm.WM_MEM_HOST if mem is None else mem,
        C.byref(par) if p == "p" else None, None, C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap, pts_out,
        out_stride, C.c_void_p(offs.ctypes.data) if off == "off" else None, cap_clusters,
        wm.WM_MEM_HOST if out_mem is None else out_mem, f if first == "first" else None,
        C.byref(m) if n_out == "n_out" else None, None, None)


@pytest.mark.parametrize("bad", [dict(ctx=None), dict(scans=None), dict(p=None), dict(first=None), dict(n_out=None),
                                 dict(null_pts=True), dict(n_scans=-1),
                                 dict(stride=8), dict(stride=10), dict(stride=14),
                                 dict(pts_out=C.c_void_p(8), out_stride=8), dict(pts_out=C.c_void_p(8), out_stride=14),
                                 dict(pts_out=C.c_void_p(8), out_stride=0), dict(mem=5), dict(out_mem=7),
                                 dict(params=dict(tolerance=0.0)), dict(params=dict(tolerance=-1.0)),
                                 dict(params=dict(tolerance=float("nan"))), dict(params=dict(tolerance=float("inf"))),
                                 dict(params=dict(min_cluster_size=-1)), dict(params=dict(max_cluster_size=-2)),
                                 dict(idx=None), dict(off=None),
                                 dict(n=0x7FFFFFF1), dict(n_scans=3, n=0x30000000),
                                 dict(n_scans=3, sizes=[0x7FFFFFF0, 0, 1]),
                                 dict(n_scans=0x1000001, n=0),
                                 # the key's budget: 4 097 scans (13 bits), one of 2^25 points (2 * 26 bits)
                                 dict(n_scans=4097, sizes=[1 << 25] + [0] * 4096)])
def test_argument_errors_without_a_device(wm, bad):
    assert call(wm, **bad) == wm.WM_ERR_ARG


def test_the_limits_admit_4096_scans_of_a_million_points():
    """The header's formula: 12 bits of scan, 21 each for a size and an index of 2^20."""
    bits = lambda v: int(v).bit_length()
    assert bits(4096 - 1) + 2 * bits(1 << 20) <= 64
    assert bits(0x1000000 - 1) + 2 * bits(1 << 20) > 64  # (what the formula refuses)


def test_no_scans_and_no_points_are_ok_without_a_device(wm):
    f = (C.c_size_t * 1)(99)
    m = C.c_size_t(5)
    off = np.full(1, 9, np.uint32)
    p = wm.cluster_params(tolerance=0.5)
    rc = wm.lib().wm_cluster_extract_batch(C.c_void_p(1), None, 0, 12, wm.WM_MEM_HOST, C.byref(p), None, None, 0, None, 0,
                                           C.c_void_p(off.ctypes.data), 0, wm.WM_MEM_HOST, f, C.byref(m), None, None)
    assert rc == wm.WM_OK and f[0] == 0 and m.value == 0 and off[0] == 0
    off[0] = 9  # offsets in device memory: not written, no device is touched
    rc = wm.lib().wm_cluster_extract_batch(C.c_void_p(1), None, 0, 12, wm.WM_MEM_HOST, C.byref(p), None, None, 0, None, 0,
                                           C.c_void_p(off.ctypes.data), 0, wm.WM_MEM_DEVICE, f, C.byref(m), None, None)
    assert rc == wm.WM_OK and f[0] == 0 and off[0] == 9
    # scans without a point: the same
    tab = (wm.ClusterScan * 3)()
    f3 = (C.c_size_t * 4)(7, 7, 7, 7)
    st = (wm.ClusterStats * 3)()
    rc = wm.lib().wm_cluster_extract_batch(C.c_void_p(1), tab, 3, 12, wm.WM_MEM_HOST, C.byref(p), None, None, 0, None, 0,
                                           C.c_void_p(off.ctypes.data), 0, wm.WM_MEM_HOST, f3, C.byref(m), st, None)
    assert rc == wm.WM_OK and list(f3) == [0, 0, 0, 0] and m.value == 0 and off[0] == 0 and st[1].n_finite == 0


def test_header_compiles_standalone(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("#include <wave/matching/cluster_extraction.hpp>\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_extract_batch_links_for_two_point_types(tmp_path):
    exe = build_exe(tmp_path, "cluster_batch_cpu.cpp", "cluster_batch_cpu")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]
    assert "cloud 1 is a null pointer" in r.stdout + r.stderr
