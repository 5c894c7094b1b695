"""The C++ drop-in wave::SACSegmentation<PointT> (include/wave/matching/sac_segmentation.hpp) on the GPU, built with g++
against the in-tree libwave_matching.so (tests/cpp_sac/sac_gpu.cpp): the scan fixture segmented with the YAML fixture's
parameters; segment() equals what the C ABI gives, byte for byte; setters and getters; a copy works on a context of
its own; a 32-byte point type; the error paths.  (Without a device: tests/test_sac_cpu.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@needs_gxx
@pytest.mark.gpu
def test_scan_segmented_through_the_class_and_the_c_abi(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "sac_gpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_sac", "sac_gpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"),
                        os.path.join(ROOT, "tests", "golden", "config", "sac_segmentation.yaml")], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
