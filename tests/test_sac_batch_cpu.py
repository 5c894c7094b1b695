"""wm_sac_segment_batch and SACSegmentation<PointT>::segmentBatch without a device: the symbol is exported, the
argument errors are found before a device is touched, empty batches are WM_OK with zero offsets and WM_NOT_CONVERGED
statuses, the header still compiles on its own and a translation unit that calls segmentBatch on pcl::PointXYZ and on
a 32-byte point type links against libwave_matching.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_sac_batch_cpp import ROOT, build_exe


def test_symbol_is_exported_and_declared(wm):
    assert "wm_sac_segment_batch" in wm.declared_symbols()
    assert hasattr(wm.lib(), "wm_sac_segment_batch")
    assert wm.WM_SAC_BATCH_MAX_POINTS == 0x7FFFFFF0 and wm.WM_SAC_BATCH_MAX_SCANS == 0x1000000
    assert C.sizeof(wm.SacScan) == 16
    header = open(os.path.join(ROOT, "include", "wavematch.h")).read()
    assert "#define WM_SAC_BATCH_MAX_POINTS 0x7FFFFFF0ull" in header
    assert "#define WM_SAC_BATCH_MAX_SCANS 0x1000000ull" in header


def call(wm, ctx=C.c_void_p(1), n_scans=2, stride=12, mem=None, params=None, scans="table", offs="offs", status="status",
         coef="coef", n=10, sizes=None, null_pts=False, cap=10, idx="idx", pts_out=None, out_stride=0, out_mem=None, p="p"):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    pts = np.zeros((4, 3), np.float32)  # (never read: every case here fails before a device is touched)
    S = max(n_scans, 0)
    rows = min(S, 5000)  # (a count beyond the limit is refused before the table is read)
    tab = (wm.SacScan * max(rows, 1))()
    for k in range(rows):
        tab[k].pts = None if null_pts else pts.ctypes.data
        tab[k].n = sizes[k] if sizes else n
    out = np.zeros(16, np.int32)
    o = (C.c_size_t * (rows + 1))()
    st = (C.c_int * max(rows, 1))()
    co = (C.c_float * (4 * max(rows, 1)))()
    par = wm.sac_params(dict(dict(distance_threshold=0.1), **(params or {})))
    return wm.lib().wm_sac_segment_batch(
        ctx, tab if scans == "table" else None, n_scans, stride, wm.WM_MEM_HOST if mem is None else mem,
        C.byref(par) if p == "p" else None, 0, co if coef == "coef" else None,
        C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap, pts_out, out_stride,
        wm.WM_MEM_HOST if out_mem is None else out_mem, o if offs == "offs" else None, None,
        st if status == "status" else None, None, None)


@pytest.mark.parametrize("bad", [dict(ctx=None), dict(scans=None), dict(p=None), dict(offs=None), dict(status=None),
                                 dict(coef=None), dict(null_pts=True), dict(n_scans=-1),
                                 dict(stride=8), dict(stride=10), dict(stride=14),
                                 dict(pts_out=C.c_void_p(8), out_stride=8), dict(pts_out=C.c_void_p(8), out_stride=14),
                                 dict(pts_out=C.c_void_p(8), out_stride=0), dict(mem=5), dict(out_mem=7),
                                 dict(params=dict(model=3)), dict(params=dict(distance_threshold=0.0)),
                                 dict(params=dict(distance_threshold=float("nan"))),
                                 dict(params=dict(distance_threshold=float("inf"))),
                                 dict(params=dict(max_iterations=0)), dict(params=dict(probability=0.0)),
                                 dict(params=dict(probability=1.0)),
                                 dict(params=dict(model=1, axis=(0, 0, 0), eps_angle=0.1)),
                                 dict(params=dict(model=2, axis=(0, 0, 1), eps_angle=0.0)),
                                 dict(params=dict(model=2, axis=(0, 0, 1), eps_angle=2.0)),
                                 dict(idx=None),
                                 dict(n=0x7FFFFFF1), dict(n_scans=3, n=0x30000000),
                                 dict(n_scans=3, sizes=[0x7FFFFFF0, 0, 1]),
                                 dict(n_scans=0x1000001, n=0)])
def test_argument_errors_without_a_device(wm, bad):
    assert call(wm, **bad) == wm.WM_ERR_ARG


def test_no_scans_and_no_samples_are_ok_without_a_device(wm):
    p = wm.sac_params(distance_threshold=0.1)
    pts = np.zeros((4, 3), np.float32)
    for out_mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
        for negative in (0, 1):
            tab = (wm.SacScan * 1)()
            o = (C.c_size_t * 1)(99)
            status = (C.c_int * 1)(5)
            coef = (C.c_float * 4)(9, 9, 9, 9)
            ms = C.c_float(3.0)
            rc = wm.lib().wm_sac_segment_batch(C.c_void_p(1), tab, 0, 12, wm.WM_MEM_HOST, C.byref(p), negative, coef, None, 0,
                                               None, 0, out_mem, o, None, status, None, C.byref(ms))
            assert rc == wm.WM_OK and o[0] == 0 and ms.value == 0.0 and status[0] == 5 and list(coef) == [9.0] * 4
            # scans of 0, 2 and 1 points: no sample anywhere
            tab = (wm.SacScan * 3)()
            for k, n in enumerate((0, 2, 1)):
                tab[k].pts, tab[k].n = pts.ctypes.data, n
            o4 = (C.c_size_t * 4)(7, 7, 7, 7)
            status = (C.c_int * 3)(5, 5, 5)
            coef = (C.c_float * 12)(*([9.0] * 12))
            st = (wm.SacStats * 3)()
            st[1].n_finite, st[1].iterations = 9, 4
            labels = np.full(3, 7, np.uint8)
            rc = wm.lib().wm_sac_segment_batch(C.c_void_p(1), tab, 3, 12, wm.WM_MEM_HOST, C.byref(p), negative, coef, None, 0,
                                               None, 0, out_mem, o4, C.c_void_p(labels.ctypes.data) if out_mem == wm.WM_MEM_HOST
                                               else None, status, st, None)
            assert rc == wm.WM_OK and list(o4) == [0, 0, 0, 0] and list(status) == [wm.WM_NOT_CONVERGED] * 3
            assert list(coef) == [9.0] * 12  # (not written)
            assert st[1].n_finite == 0 and st[1].iterations == 0 and [s.best_hypothesis for s in st] == [-1] * 3
            if out_mem == wm.WM_MEM_HOST:
                assert (labels == wm.WM_SAC_NONE).all()


def test_header_compiles_standalone(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("#include <wave/matching/sac_segmentation.hpp>\n"
                   "template <class C> void use(wave::SACSegmentation<pcl::PointXYZ> &f, const C &in,\n"
                   "                            std::vector<pcl::PointIndices> &i, std::vector<pcl::ModelCoefficients> &c)\n"
                   "{ f.segmentBatch(in, i, c); }\n"
                   "void call(wave::SACSegmentation<pcl::PointXYZ> &f,\n"
                   "          const std::vector<wave::SACSegmentation<pcl::PointXYZ>::PointCloudConstPtr> &in,\n"
                   "          std::vector<pcl::PointIndices> &i, std::vector<pcl::ModelCoefficients> &c) { use(f, in, i, c); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_segment_batch_links_for_two_point_types(tmp_path):
    exe = build_exe(tmp_path, "sac_batch_cpu.cpp", "sac_batch_cpu")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]
    assert "cloud 1 is a null pointer" in r.stdout + r.stderr
