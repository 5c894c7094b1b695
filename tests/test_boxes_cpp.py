"""The C++ drop-in wave::ClusterBoxes<PointT> (include/wave/matching/cluster_boxes.hpp) on the GPU, built with g++
against the in-tree libwave_matching.so (tests/cpp_boxes/boxes_gpu.cpp): the scan fixture clustered with the YAML
fixture's parameters; compute() equals the bytes of the C ABI; computeBatch over four clouds equals four compute()
calls; setters, the copy, the accessors, a null cloud among the batch.  Without a device: the headers compile alone and
the class is constructed, copied and destroyed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
HEADERS = ["wave/matching/cluster_boxes.hpp", "wave/matching/impl/cluster_boxes.hpp"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@needs_gxx
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_standalone(tmp_path, header):
    src = tmp_path / "one.cpp"
    src.write_text("#include <%s>\n" % header)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_construction_and_copies_without_a_device(tmp_path):
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "boxes_cpu.cpp"
    src.write_text("""
#include <cstdio>
#include "wave/matching/cluster_boxes.hpp"
int main() {
    wave::ClusterBoxes<pcl::PointXYZ> a;
    a.setClusters(std::vector<pcl::PointIndices>(3));
    wave::ClusterBoxes<pcl::PointXYZ> b = a, c;
    c = b;
    std::vector<wave::ClusterBox> out(2);
    c.compute(out);  // no input cloud: nothing to do, no device needed
    wave::ClusterBox box;
    float l0, l1, l2;
    const bool ok = out.empty() && c.getClusters().size() == 3 && !c.getInputCloud() && !box.getEigenValues(l0, l1, l2) &&
                    sizeof(box) == 128;
    std::printf("failed checks: %d\\n", ok ? 0 : 1);
    return ok ? 0 : 1;
}
""")
    exe = str(tmp_path / "boxes_cpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                        exe, "-L" + LIB, "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


@needs_gxx
@pytest.mark.gpu
def test_scan_boxes_through_the_class_and_the_c_abi(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "boxes_gpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_boxes", "boxes_gpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"),
                        os.path.join(ROOT, "tests", "golden", "config", "cluster_extraction.yaml")], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
