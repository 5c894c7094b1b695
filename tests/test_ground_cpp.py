"""The C++ drop-in wave::GroundSegmentation<PointT> (include/wave/matching/ground_segmentation.hpp), built with g++
against the in-tree libwave_matching.so.  CPU: every header compiles on its own, the YAML constructor, construction
without a device.  GPU: the reference's how_to_use flow, whose three clouds must be the checker's
(tests/ground_reference.py) lists, point for point and in order."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_reference as G  # noqa: E402
import ground_scenes as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
HEADERS = ["wave/matching/ground_segmentation.hpp", "wave/matching/ground_segmentation_params.hpp",
           "wave/matching/impl/ground_segmentation.hpp", "wave/compat/pcl_filter_min.hpp"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, src, name):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_ground", src), "-o", exe, "-L" + LIB, "-lwave_matching",
                        "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


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
    exe = _build(tmp_path, "ground_cpu.cpp", "ground_cpu")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, S.YAML], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


@needs_gxx
@pytest.mark.gpu
def test_how_to_use_flow(tmp_path, testscan):
    exe = _build(tmp_path, "ground_gpu.cpp", "ground_gpu")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"), S.YAML, str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
    pts = G.car_box_removal(testscan)
    ref = G.segment(pts, G.load_yaml(S.YAML))
    assert ref["margin"] > 1e-9 and ref["bin_margin"] > 1e-9
    for name in ("ground", "obstacle", "overhanging"):
        got = np.fromfile(str(tmp_path / (name + ".bin")), np.float32).reshape(-1, 3)
        np.testing.assert_array_equal(got, pts[ref[name]], err_msg=name)
