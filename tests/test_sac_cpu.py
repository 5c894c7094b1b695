"""wm_sac_segment and wave::SACSegmentation<PointT> without a device: the symbols are exported and declared, the
structures have the header's layout, every argument error is found before a device is touched, a cloud of fewer than
three records has no model without a device, the headers compile on their own, and tests/cpp_sac/sac_cpu.cpp
(parameter loading and the class's error paths) runs with no device visible."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
YAML = os.path.join(ROOT, "tests", "golden", "config", "sac_segmentation.yaml")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_symbols_are_exported_and_declared(wm):
    for name in ("wm_sac_segment", "wm_sac_default_params"):
        assert name in wm.declared_symbols() and hasattr(wm.lib(), name)
    assert (wm.WM_SAC_PLANE, wm.WM_SAC_PERPENDICULAR_PLANE, wm.WM_SAC_PARALLEL_PLANE) == (0, 1, 2)
    assert (wm.WM_SAC_NONE, wm.WM_SAC_INLIER, wm.WM_SAC_OUTLIER) == (0, 1, 2)
    assert C.sizeof(wm.SacParams) == 80 and C.sizeof(wm.SacStats) == 80
    p = wm.sac_params()
    assert (p.model, p.distance_threshold, p.max_iterations, p.probability, p.optimize_coefficients, p.seed) == \
        (0, 0.0, 50, 0.99, 1, 0)
    p = wm.sac_params(dict(max_iterations=7), axis=(1, 2, 3), seed=2 ** 63 + 5)
    assert p.max_iterations == 7 and list(p.axis) == [1.0, 2.0, 3.0] and p.seed == 2 ** 63 + 5
    with pytest.raises(AttributeError):
        wm.sac_params(tolerance=1.0)


def call(wm, ctx=C.c_void_p(1), n=10, stride=12, mem=None, out_mem=None, params="p", coef="coef", n_out="n_out", cap=10,
         idx="idx", pts="pts", **fields):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    cloud = np.zeros((10, 4), np.float32)
    out = np.zeros(16, np.int32)
    m = C.c_size_t(77)
    co = (C.c_float * 4)()
    p = wm.sac_params(dict(dict(distance_threshold=0.1), **fields))
    rc = wm.lib().wm_sac_segment(
        ctx, C.c_void_p(cloud.ctypes.data) if pts == "pts" else None, n, stride, wm.WM_MEM_HOST if mem is None else mem,
        C.byref(p) if params == "p" else None, co if coef == "coef" else None,
        C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap, wm.WM_MEM_HOST if out_mem is None else out_mem,
        C.byref(m) if n_out == "n_out" else None, None, None)
    return rc, m.value


AXIS = dict(model=1, axis=(0, 0, 1), eps_angle=0.1)


@pytest.mark.parametrize("bad", [
    dict(ctx=None), dict(params=None), dict(coef=None), dict(n_out=None), dict(pts=None), dict(idx=None),
    dict(stride=8), dict(stride=10), dict(stride=14), dict(mem=5), dict(out_mem=7), dict(n=0x7FFFFFF1),
    dict(model=3), dict(model=-1),
    dict(distance_threshold=0.0), dict(distance_threshold=-1.0), dict(distance_threshold=float("nan")),
    dict(distance_threshold=float("inf")),
    dict(max_iterations=0), dict(max_iterations=-5),
    dict(probability=0.0), dict(probability=1.0), dict(probability=-0.5), dict(probability=float("nan")),
    dict(AXIS, axis=(0, 0, 0)), dict(AXIS, axis=(float("nan"), 0, 1)), dict(AXIS, axis=(float("inf"), 0, 1)),
    dict(AXIS, eps_angle=0.0), dict(AXIS, eps_angle=-0.1), dict(AXIS, eps_angle=math.pi / 2 + 1e-9),
    dict(AXIS, eps_angle=float("nan")), dict(AXIS, model=2, eps_angle=0.0), dict(AXIS, model=2, axis=(0, 0, 0)),
], ids=lambda b: "-".join("%s=%s" % kv for kv in sorted(b.items(), key=lambda kv: kv[0]) if kv[0] not in ("axis",))[:60])
def test_argument_errors_without_a_device(wm, bad):
    rc, m = call(wm, **bad)
    assert rc == wm.WM_ERR_ARG
    assert m == 77  # nothing is written


@pytest.mark.parametrize("n", [0, 1, 2])
def test_fewer_than_three_records_have_no_model_without_a_device(wm, n):
    rc, m = call(wm, n=n)
    assert rc == wm.WM_NOT_CONVERGED and m == 0
    rc, m = call(wm, n=n, pts=None if n == 0 else "pts", cap=0, idx=None, **dict(AXIS, eps_angle=math.pi / 2))
    assert rc == wm.WM_NOT_CONVERGED and m == 0
    st = wm.SacStats()
    st.iterations = 9
    p = wm.sac_params(distance_threshold=0.1)
    m, co = C.c_size_t(5), (C.c_float * 4)()
    cloud = np.zeros((4, 3), np.float32)
    rc = wm.lib().wm_sac_segment(C.c_void_p(1), C.c_void_p(cloud.ctypes.data), n, 12, wm.WM_MEM_HOST, C.byref(p), co, None, 0,
                                 wm.WM_MEM_DEVICE, C.byref(m), None, C.byref(st))
    assert rc == wm.WM_NOT_CONVERGED and m.value == 0
    assert (st.iterations, st.skipped, st.rounds, st.hypotheses, st.best_hypothesis, st.n_finite) == (0, 0, 0, 0, -1, 0)


def test_the_option_is_in_the_table():
    src = open(os.path.join(LIB, "csrc", "wm_ctx.hip")).read()
    assert '{"sac_round", "WM_TUNE_SAC_ROUND", &wm_ctx::tune_sac_round, nullptr, 1, 1024, 0}' in src


@needs_gxx
@pytest.mark.parametrize("header", ["wave/matching/sac_segmentation.hpp", "wave/matching/impl/sac_segmentation.hpp",
                                    "wave/compat/pcl_model_coefficients_min.hpp"])
def test_headers_compile_standalone(tmp_path, header):
    src = tmp_path / "one.cpp"
    src.write_text("#include <%s>\n" % header)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_yaml_construction_and_error_paths_without_a_device(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "sac_cpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_sac", "sac_cpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, YAML], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]
    assert "only the plane models are built" in r.stdout + r.stderr
