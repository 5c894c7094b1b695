"""GroundSegmentation<PointT>::filterBatch (include/wave/matching/ground_segmentation.hpp) on the GPU: the outputs of
one batched call over a drive of the fixture equal those of eight filter() calls, point for point and field for field,
for pcl::PointXYZ and a 32-byte point type (tests/cpp_ground/ground_batch_gpu.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
YAML = os.path.join(ROOT, "tests", "golden", "config", "ground_segmentation.yaml")


def build_exe(tmp_path, src, name):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_ground", src), "-o", exe, "-L" + LIB, "-lwave_matching",
                        "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.gpu
def test_filter_batch_equals_eight_filters(tmp_path):
    exe = build_exe(tmp_path, "ground_batch_gpu.cpp", "ground_batch_gpu")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"), YAML], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
    assert "input 1 is null" in r.stdout + r.stderr
