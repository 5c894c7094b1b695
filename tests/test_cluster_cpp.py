"""The C++ drop-in wave::EuclideanClusterExtraction<PointT> (include/wave/matching/cluster_extraction.hpp) on the GPU,
built with g++ against the in-tree libwave_matching.so (tests/cpp_cluster/cluster_gpu.cpp): the scan fixture clustered
with the YAML fixture's parameters; extract() equals the clusters the C ABI gives; setters and getters; a copy works on
a context of its own.  (Without a device: tests/test_cluster_reference_cpu.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@needs_gxx
@pytest.mark.gpu
def test_scan_clustered_through_the_class_and_the_c_abi(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "cluster_gpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_cluster", "cluster_gpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"),
                        os.path.join(ROOT, "tests", "golden", "config", "cluster_extraction.yaml")], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
