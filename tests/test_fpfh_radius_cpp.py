"""wave::FPFHEstimation<PointT> with setRadiusSearch (include/wave/matching/fpfh.hpp), built with g++ against the in-tree
libwave_matching.so the way tests/test_fpfh_cpp.py builds its case.  Without a device: the headers compile alone, the
class is constructed, copied and destroyed with the new setters, and the radius YAML fixture loads.  On the GPU
(tests/cpp_fpfh_radius/fpfh_radius_gpu.cpp): compute() equals the bytes of wm_fpfh_radius on the scan fixture with the
YAML fixture's radii; a radius and a k both set by the caller give an empty result."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
HEADERS = ["wave/matching/fpfh.hpp", "wave/matching/impl/fpfh.hpp", "wavematch.h"]
YAML = os.path.join(ROOT, "tests", "golden", "config", "fpfh_radius.yaml")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(src, exe):
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                        exe, "-L" + LIB, "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


@needs_gxx
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_standalone(tmp_path, header):
    src = tmp_path / "one.cpp"
    src.write_text("#include <%s>\n" % header)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_construction_copies_and_the_yaml_without_a_device(tmp_path):
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "fpfh_radius_cpu.cpp"
    src.write_text("""
#include <cstdio>
#include "wave/matching/fpfh.hpp"
#include "wavematch.h"
int main(int, char **argv) {
    wave::FPFHEstimation<pcl::PointXYZ> a;
    const bool fresh = a.getRadiusSearch() == 0.0 && a.getNormalRadiusSearch() == 0.0 && a.getKSearch() == 10 &&
                       a.getNormalKSearch() == 10;  // the defaults stay k = 10 / 10
    a.setRadiusSearch(0.8);
    a.setNormalRadiusSearch(0.4);
    wave::FPFHEstimation<pcl::PointXYZ> b = a, c;
    c = b;
    std::vector<pcl::FPFHSignature33> out(2);
    c.compute(out);  // no input cloud: nothing to do, no device needed
    wave::FPFHParams radius(argv[1]), k(argv[2]), missing("/nonexistent/fpfh.yaml");
    const bool ok = fresh && out.empty() && c.getRadiusSearch() == 0.8 && c.getNormalRadiusSearch() == 0.4 && !c.getInputCloud() &&
                    radius.feature_radius == 1.0 && radius.normal_radius == 0.5 && radius.feature_k == 10 && radius.normal_k == 10 &&
                    k.feature_k == 12 && k.normal_k == 16 && k.feature_radius == 0.0 && k.normal_radius == 0.0 &&
                    missing.feature_k == 10 && missing.feature_radius == 0.0;
    // the host finish of a radius normal needs no device either
    const int64_t u = 1ll << 36, sums[9] = {0, u / 2, 0, u / 2, 0, 0, u / 4, 0, 0};
    const float p[3] = {0.f, 0.f, 5.f};
    float n[4] = {9.f, 9.f, 9.f, 9.f};
    const bool host = wm_normal_from_sums(sums, 4, 0, p, n) == WM_OK && n[0] == 0.f && n[1] == 0.f && n[2] == -1.f && n[3] == 0.f &&
                      wm_normal_from_sums(sums, 2, 0, p, n) == WM_OK && n[2] == 0.f && wm_normal_from_sums(nullptr, 4, 0, p, n) == WM_ERR_ARG;
    std::printf("failed checks: %d\\n", (ok ? 0 : 1) + (host ? 0 : 1));
    return ok && host ? 0 : 1;
}
""")
    exe = str(tmp_path / "fpfh_radius_cpu")
    _build(src, exe)
    r = subprocess.run([exe, YAML, os.path.join(ROOT, "tests", "golden", "config", "fpfh.yaml")], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


@needs_gxx
@pytest.mark.gpu
def test_scan_descriptors_through_the_class_and_the_c_abi(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "fpfh_radius_gpu")
    _build(os.path.join(ROOT, "tests", "cpp_fpfh_radius", "fpfh_radius_gpu.cpp"), exe)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"), YAML], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
