"""wm_cluster_boxes: what can be checked without a device -- the argument errors, which come before a device is touched
(the context is a pointer that must never be followed), the empty call, and the Python surface."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(wm, ctx=C.c_void_p(1), n=10, stride=16, mem=None, list_mem=None, out_mem=None, pts="pts", idx="idx", off="off",
          out="out", n_members=10, n_clusters=2):
    cloud = np.zeros((10, 4), np.float32)
    indices = np.arange(10, dtype=np.int32)
    offsets = np.array([0, 5, 10], np.uint32)
    boxes = np.zeros(2, wm.BOX_DTYPE)
    host = wm.WM_MEM_HOST
    return wm.lib().wm_cluster_boxes(
        ctx, C.c_void_p(cloud.ctypes.data) if pts == "pts" else None, n, stride, host if mem is None else mem,
        C.c_void_p(indices.ctypes.data) if idx == "idx" else None, n_members,
        C.c_void_p(offsets.ctypes.data) if off == "off" else None, n_clusters, host if list_mem is None else list_mem,
        C.c_void_p(boxes.ctypes.data) if out == "out" else None, host if out_mem is None else out_mem, None)


@pytest.mark.parametrize("bad", [dict(ctx=None), dict(off=None), dict(out=None), dict(stride=8), dict(stride=10),
                                 dict(stride=14), dict(mem=5), dict(list_mem=3), dict(out_mem=7), dict(n=0x7FFFFFF1),
                                 dict(n_members=0x7FFFFFF1), dict(pts=None), dict(idx=None, n_members=9),
                                 dict(idx=None, n_members=11), dict(ctx=None, n_clusters=0)])
def test_argument_errors_without_a_device(wm, bad):
    assert _call(wm, **bad) == wm.WM_ERR_ARG


def test_no_clusters_is_ok_without_a_device(wm):
    assert _call(wm, n_clusters=0) == wm.WM_OK
    assert _call(wm, n_clusters=0, off=None, out=None) == wm.WM_OK
    assert _call(wm, n_clusters=0, idx=None, pts=None, n=0, n_members=0, mem=wm.WM_MEM_DEVICE,
                 list_mem=wm.WM_MEM_DEVICE, out_mem=wm.WM_MEM_DEVICE) == wm.WM_OK
    ms = C.c_float(7)
    assert wm.lib().wm_cluster_boxes(C.c_void_p(1), None, 0, 12, 0, None, 0, None, 0, 0, None, 0, C.byref(ms)) == wm.WM_OK
    assert ms.value == 0.0


def test_symbol_struct_and_the_python_surface(wm):
    assert "wm_cluster_boxes" in wm.declared_symbols()
    assert C.sizeof(wm.ClusterBox) == 128 and wm.BOX_DTYPE.itemsize == 128
    for name, _ in wm.ClusterBox._fields_:  # the two declarations agree field by field
        assert getattr(wm.ClusterBox, name).offset == wm.BOX_DTYPE.fields[name][1], name
    assert (wm.WM_BOX_EMPTY, wm.WM_BOX_NONFINITE, wm.WM_BOX_RANGE) == (1, 2, 4)
    hdr = open(os.path.join(ROOT, "include", "wavematch.h")).read()
    assert "WM_BOX_EMPTY = 1, WM_BOX_NONFINITE = 2, WM_BOX_RANGE = 4" in hdr
    assert hasattr(wm.Context, "cluster_boxes")
