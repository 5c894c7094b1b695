"""wm_ground_segment_batch and GroundSegmentation<PointT>::filterBatch without a device: the symbol is exported, the
argument errors are found before a device is touched, the header still compiles on its own and a translation unit that
calls filterBatch on pcl::PointXYZ and on a 32-byte point type links against libwave_matching.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_ground_batch_cpp import ROOT, build_exe


def test_symbol_is_exported_and_declared(wm):
    assert "wm_ground_segment_batch" in wm.declared_symbols()
    assert hasattr(wm.lib(), "wm_ground_segment_batch")
    assert wm.WM_GROUND_BATCH_MAX_KEYS == 0xFFFFFFFF and wm.WM_GROUND_BATCH_MAX_POINTS == 0x7FFFFFF0


def call(wm, ctx=C.c_void_p(1), n_scans=1, stride=12, mem=None, keep=6, params=None, scans="table", offs="offs",
         n=10, cap=10, pts_out=None, out_stride=0, out_mem=None):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    pts = np.zeros((max(n, 1) if n < 1000 else 1, 3), np.float32)
    tab = (wm.GroundScan * max(n_scans, 1))()
    for k in range(max(n_scans, 0)):
        tab[k].pts, tab[k].n = pts.ctypes.data, n
    out = np.zeros(max(cap, 1), np.int32)
    o = (C.c_size_t * (max(n_scans, 0) + 1))()
    p = wm.ground_params(params)
    return wm.lib().wm_ground_segment_batch(
        ctx, tab if scans == "table" else None, n_scans, stride, wm.WM_MEM_HOST if mem is None else mem, C.byref(p),
        keep, C.c_void_p(out.ctypes.data), cap, pts_out, out_stride, wm.WM_MEM_HOST if out_mem is None else out_mem,
        o if offs == "offs" else None, None, None, None)


@pytest.mark.parametrize("bad", [dict(ctx=None), dict(n_scans=-1), dict(stride=10), dict(keep=8),
                                 dict(params=dict(num_bins_a=0)), dict(stride=8), dict(stride=14), dict(keep=-1),
                                 dict(mem=5), dict(out_mem=7), dict(scans=None), dict(offs=None),
                                 dict(params=dict(p_sn=0.0)), dict(params=dict(rmax=float("nan"))),
                                 dict(pts_out=C.c_void_p(8), out_stride=10),
                                 dict(n=0x7FFFFFF1), dict(n_scans=3, n=0x30000000),
                                 dict(n_scans=300, params=dict(num_bins_a=4096, num_bins_l=4096))])
def test_argument_errors_without_a_device(wm, bad):
    assert call(wm, **bad) == wm.WM_ERR_ARG


def test_no_scans_is_ok_without_a_device(wm):
    o = (C.c_size_t * 1)(99)
    p = wm.ground_params()
    rc = wm.lib().wm_ground_segment_batch(C.c_void_p(1), None, 0, 12, wm.WM_MEM_HOST, C.byref(p), 6, None, 0, None, 0,
                                          wm.WM_MEM_HOST, o, None, None, None)
    assert rc == wm.WM_OK and o[0] == 0


def test_header_compiles_standalone(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("#include <wave/matching/ground_segmentation.hpp>\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_filter_batch_links_for_two_point_types(tmp_path):
    exe = build_exe(tmp_path, "ground_batch_cpu.cpp", "ground_batch_cpu")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]
