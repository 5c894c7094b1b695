"""SACSegmentation<PointT>::segmentBatch (include/wave/matching/sac_segmentation.hpp) on the GPU: one batched call over
the scan fixture cut into four sub-clouds equals four segment() calls, for pcl::PointXYZ and a 32-byte point type, with
and without the refit; a copy works on a context of its own; empty vectors, empty clouds and clouds without a model; a
null cloud is logged (tests/cpp_sac/sac_batch_gpu.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
YAML = os.path.join(ROOT, "tests", "golden", "config", "sac_segmentation.yaml")


def build_exe(tmp_path, src, name):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_sac", src), "-o", exe, "-L" + LIB, "-lwave_matching",
                        "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.gpu
def test_segment_batch_equals_four_segments(tmp_path):
    exe = build_exe(tmp_path, "sac_batch_gpu.cpp", "sac_batch_gpu")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"), YAML], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
    assert "cloud 1 is a null pointer" in r.stdout + r.stderr
