"""The C++ drop-ins wave::FPFHEstimation<PointT> and wave::matchFeatures (include/wave/matching/fpfh.hpp) on the GPU,
built with g++ against the in-tree libwave_matching.so (tests/cpp_fpfh/fpfh_gpu.cpp): the scan fixture with the YAML
fixture's parameters; compute() equals the bytes of the C ABI; the caller's normals, the copy, a 32-byte point type;
matchFeatures equals wm_feature_match minus the unmatched rows.  Without a device: the headers compile alone and the
class is constructed, copied and destroyed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
HEADERS = ["wave/matching/fpfh.hpp", "wave/matching/impl/fpfh.hpp", "wave/compat/pcl_fpfh_min.hpp"]

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
    src = tmp_path / "fpfh_cpu.cpp"
    src.write_text("""
#include <cstdio>
#include "wave/matching/fpfh.hpp"
int main() {
    wave::FPFHEstimation<pcl::PointXYZ> a;
    a.setKSearch(17);
    a.setNormalKSearch(8);
    wave::FPFHEstimation<pcl::PointXYZ> b = a, c;
    c = b;
    std::vector<pcl::FPFHSignature33> out(2);
    c.compute(out);  // no input cloud: nothing to do, no device needed
    std::vector<pcl::Correspondence> corr(1);
    const bool matched = wave::matchFeatures(std::vector<pcl::FPFHSignature33>(), out, true, corr);  // no rows: no device either
    wave::FPFHParams missing("/nonexistent/fpfh.yaml");  // logs, keeps the defaults
    pcl::FPFHSignature33 d;
    const bool ok = out.empty() && c.getKSearch() == 17 && c.getNormalKSearch() == 8 && !c.getInputCloud() && matched &&
                    corr.empty() && missing.feature_k == 10 && missing.normal_k == 10 && sizeof(d.histogram) == 132;
    std::printf("failed checks: %d\\n", ok ? 0 : 1);
    return ok ? 0 : 1;
}
""")
    exe = str(tmp_path / "fpfh_cpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                        exe, "-L" + LIB, "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


@needs_gxx
@pytest.mark.gpu
def test_scan_descriptors_through_the_class_and_the_c_abi(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "fpfh_gpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_fpfh", "fpfh_gpu.cpp"), "-o", exe, "-L" + LIB,
                        "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"),
                        os.path.join(ROOT, "tests", "golden", "config", "fpfh.yaml")], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
