"""The C++ drop-in wave::ConditionalEuclideanClustering<PointT> (include/wave/matching/conditional_clustering.hpp),
built with g++ against the in-tree libwave_matching.so.

On the GPU (tests/cpp_cluster_cond/cluster_cond_gpu.cpp): the scan fixture segmented with the YAML fixture's
parameters; segment() equals the clusters the C ABI gives; setNormalKSearch against wm_estimate_normals' output;
setInputAttributes with a 32-byte stride; clearConditions() against EuclideanClusterExtraction::extract; a copy works on
a context of its own; the error paths give no clusters.
Without a device (tests/cpp_cluster_cond/cluster_cond_cpu.cpp): the headers compile alone, the YAML constructor,
construction, setters and copies."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
YAML = os.path.join(ROOT, "tests", "golden", "config", "conditional_clustering.yaml")
HEADERS = ["wave/matching/conditional_clustering.hpp", "wave/matching/impl/conditional_clustering.hpp"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_cluster_cond", name + ".cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@needs_gxx
@pytest.mark.gpu
def test_scan_segmented_through_the_class_and_the_c_abi(tmp_path):
    exe = _build(tmp_path, "cluster_cond_gpu")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"), YAML], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]


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
    exe = _build(tmp_path, "cluster_cond_cpu")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, YAML], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]
