"""The C++ drop-in wave::CorrespondenceRejectorSampleConsensus<PointT>
(include/wave/matching/correspondence_rejection.hpp) on the GPU, built with g++ against the in-tree libwave_matching.so
(tests/cpp_corr_ransac/corr_ransac_gpu.cpp): the pipeline through FPFHEstimation and matchFeatures on the scan fixture
with the YAML fixture's parameters; the class equals the bytes of the C ABI; a copy, a 32-byte point type, and the
no-model path that returns the input and the identity."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.gpu
def test_the_pipeline_through_the_class_and_the_c_abi(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "corr_ransac_gpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_corr_ransac", "corr_ransac_gpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"),
                        os.path.join(ROOT, "tests", "golden", "config", "correspondence_rejection.yaml")],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
