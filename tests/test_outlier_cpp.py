"""The C++ drop-in wave::OutlierRemoval<PointT> (include/wave/matching/outlier_removal.hpp) on the GPU, built with g++
against the in-tree libwave_matching.so (tests/cpp_outlier/outlier_gpu.cpp): the scan fixture filtered with the YAML
fixture's parameters, into a second cloud and in place, both filters and both settings of setNegative; every kept
cloud is pcl::copyPointCloud of the indices the C ABI keeps.  (Without a device: tests/test_outlier_reference_cpu.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@needs_gxx
@pytest.mark.gpu
def test_scan_filtered_in_place_and_into_a_second_cloud(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "outlier_gpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_outlier", "outlier_gpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"),
                        os.path.join(ROOT, "tests", "golden", "config", "outlier_removal.yaml")], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
