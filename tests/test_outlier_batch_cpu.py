"""wm_outlier_filter_batch and OutlierRemoval<PointT>::filterBatch without a device: the symbol is exported, the
argument errors are found before a device is touched, empty batches are WM_OK with zero offsets, the header still
compiles on its own and a translation unit that calls filterBatch on pcl::PointXYZ and on a 32-byte point type links
against libwave_matching.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_outlier_batch_cpp import ROOT, build_exe


def test_symbol_is_exported_and_declared(wm):
    assert "wm_outlier_filter_batch" in wm.declared_symbols()
    assert hasattr(wm.lib(), "wm_outlier_filter_batch")
    assert wm.WM_OUTLIER_BATCH_MAX_POINTS == 0x7FFFFFF0 and wm.WM_OUTLIER_BATCH_MAX_SCANS == 0x1000000
    assert C.sizeof(wm.OutlierScan) == 16
    header = open(os.path.join(ROOT, "include", "wavematch.h")).read()
    assert "#define WM_OUTLIER_BATCH_MAX_POINTS 0x7FFFFFF0ull" in header
    assert "#define WM_OUTLIER_BATCH_MAX_SCANS 0x1000000ull" in header


def call(wm, ctx=C.c_void_p(1), n_scans=2, stride=12, mem=None, params=None, scans="table", offs="offs", status="status",
         n=10, sizes=None, null_pts=False, cap=10, idx="idx", pts_out=None, out_stride=0, out_mem=None, p="p"):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    pts = np.zeros((4, 3), np.float32)  # (never read: every case here fails before, or touches nothing)
    S = max(n_scans, 0)
    rows = min(S, 5000)  # (a count beyond the limit is refused before the table is read)
    tab = (wm.OutlierScan * max(rows, 1))()
    for k in range(rows):
        tab[k].pts = None if null_pts else pts.ctypes.data
        tab[k].n = sizes[k] if sizes else n
    out = np.zeros(16, np.int32)
    o = (C.c_size_t * (rows + 1))()
    st = (C.c_int * max(rows, 1))()
    par = wm.outlier_params(dict(dict(method=0, mean_k=8, stddev_mult=1.0, radius=0.5, min_neighbors=5), **(params or {})))
    return wm.lib().wm_outlier_filter_batch(
        ctx, tab if scans == "table" else None, n_scans, stride, wm.WM_MEM_HOST if mem is None else mem,
        C.byref(par) if p == "p" else None, C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap, pts_out,
        out_stride, wm.WM_MEM_HOST if out_mem is None else out_mem, o if offs == "offs" else None, None, None, None,
        st if status == "status" else None, None, None)


@pytest.mark.parametrize("bad", [dict(ctx=None), dict(scans=None), dict(p=None), dict(offs=None), dict(status=None),
                                 dict(null_pts=True), dict(n_scans=-1),
                                 dict(stride=8), dict(stride=10), dict(stride=14),
                                 dict(pts_out=C.c_void_p(8), out_stride=8), dict(pts_out=C.c_void_p(8), out_stride=14),
                                 dict(pts_out=C.c_void_p(8), out_stride=0), dict(mem=5), dict(out_mem=7),
                                 dict(params=dict(method=2)), dict(params=dict(mean_k=0)), dict(params=dict(mean_k=32)),
                                 dict(params=dict(method=1, radius=0.0)), dict(params=dict(method=1, radius=-1.0)),
                                 dict(params=dict(method=1, radius=float("nan"))),
                                 dict(params=dict(method=1, radius=float("inf"))),
                                 dict(params=dict(method=1, min_neighbors=-1)),
                                 dict(idx=None),
                                 dict(n=0x7FFFFFF1), dict(n_scans=3, n=0x30000000),
                                 dict(n_scans=3, sizes=[0x7FFFFFF0, 0, 1]),
                                 dict(n_scans=0x1000001, n=0)])
def test_argument_errors_without_a_device(wm, bad):
    assert call(wm, **bad) == wm.WM_ERR_ARG


def test_no_scans_and_no_points_are_ok_without_a_device(wm):
    p = wm.outlier_params(method=0, mean_k=8, stddev_mult=1.0)
    for out_mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
        o = (C.c_size_t * 1)(99)
        ms = C.c_float(3.0)
        rc = wm.lib().wm_outlier_filter_batch(C.c_void_p(1), None, 0, 12, wm.WM_MEM_HOST, C.byref(p), None, 0, None, 0,
                                              out_mem, o, None, None, None, None, None, C.byref(ms))
        assert rc == wm.WM_OK and o[0] == 0 and ms.value == 0.0
    # scans without a point: the same, every status WM_OK and every stats entry zero
    for method in (0, 1):
        p = wm.outlier_params(method=method, mean_k=8, stddev_mult=1.0, radius=0.5, min_neighbors=5)
        tab = (wm.OutlierScan * 3)()
        o3 = (C.c_size_t * 4)(7, 7, 7, 7)
        status = (C.c_int * 3)(5, 5, 5)
        st = (wm.OutlierStats * 3)()
        st[1].n_finite = 9
        rc = wm.lib().wm_outlier_filter_batch(C.c_void_p(1), tab, 3, 12, wm.WM_MEM_HOST, C.byref(p), None, 0, None, 0,
                                              wm.WM_MEM_HOST, o3, None, None, None, status, st, None)
        assert rc == wm.WM_OK and list(o3) == [0, 0, 0, 0] and list(status) == [wm.WM_OK] * 3 and st[1].n_finite == 0


def test_header_compiles_standalone(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("#include <wave/matching/outlier_removal.hpp>\n"
                   "template <class C> void use(wave::OutlierRemoval<pcl::PointXYZ> &f, const C &in,\n"
                   "                            std::vector<pcl::PointCloud<pcl::PointXYZ>> &out) { f.filterBatch(in, out); }\n"
                   "void call(wave::OutlierRemoval<pcl::PointXYZ> &f,\n"
                   "          const std::vector<wave::OutlierRemoval<pcl::PointXYZ>::PointCloudConstPtr> &in,\n"
                   "          std::vector<pcl::PointCloud<pcl::PointXYZ>> &out) { use(f, in, out); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_filter_batch_links_for_two_point_types(tmp_path):
    exe = build_exe(tmp_path, "outlier_batch_cpu.cpp", "outlier_batch_cpu")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]
    assert "cloud 1 is a null pointer" in r.stdout + r.stderr
