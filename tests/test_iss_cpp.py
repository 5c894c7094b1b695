"""The C++ drop-in wave::ISSKeypoint3D<PointT> (include/wave/matching/iss_keypoints.hpp), built with g++ against the
in-tree libwave_matching.so.  On the GPU (tests/cpp_iss/iss_gpu.cpp): compute() on the scan fixture with the YAML
fixture's parameters equals the C ABI's bytes; a copy, a 32-byte point type and the refused setters.  Without a device:
the headers compile on their own, and the class is constructed, copied, reads its YAML file and runs its empty and
refused paths with no device visible."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")
YAML = os.path.join(ROOT, "tests", "golden", "config", "iss_keypoints.yaml")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build(src, exe):
    import __graft_entry__ as g
    g.build()
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                        exe, "-L" + LIB, "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


@needs_gxx
@pytest.mark.gpu
def test_compute_on_the_scan_equals_the_c_abi(tmp_path):
    exe = str(tmp_path / "iss_gpu")
    build(os.path.join(ROOT, "tests", "cpp_iss", "iss_gpu.cpp"), exe)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "testscan.pcd"), YAML], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]


@needs_gxx
@pytest.mark.parametrize("header", ["wave/matching/iss_keypoints.hpp", "wave/matching/impl/iss_keypoints.hpp"])
def test_headers_compile_standalone(tmp_path, header):
    src = tmp_path / "one.cpp"
    src.write_text("#include <%s>\n" % header)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_the_rule_header_compiles_with_a_plain_compiler(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text('#include "wm_iss_rule.hpp"\nint main() { const long long s[6] = {4, 0, 0, 2, 0, 1};\n'
                   "return wm::iss_third(s, 9, 5, 36, 0.975, 0.975) == 1.0 ? 0 : 1; }\n")
    exe = str(tmp_path / "one")
    r = subprocess.run(["g++", "-std=c++14", "-ffp-contract=off", "-I" + os.path.join(LIB, "csrc"), str(src), "-o", exe, "-lm"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert subprocess.run([exe], timeout=60).returncode == 0


@needs_gxx
def test_construction_copies_and_the_paths_without_a_device(tmp_path):
    src = tmp_path / "iss_cpu.cpp"
    src.write_text("""
#include <cstdio>
#include "wave/matching/iss_keypoints.hpp"
int main(int argc, char **argv) {
    using Cloud = pcl::PointCloud<pcl::PointXYZ>;
    wave::ISSKeypoint3D<pcl::PointXYZ> a;
    a.setSalientRadius(2.0);
    a.setNonMaxRadius(1.5);
    a.setThreshold21(0.9);
    a.setThreshold32(0.8);
    a.setMinNeighbors(7);
    wave::ISSKeypoint3D<pcl::PointXYZ> b = a, c;
    c = b;
    const wave::ISSKeypointParams &p = c.getParams();
    bool ok = p.salient_radius == 2.0 && p.non_max_radius == 1.5 && p.gamma_21 == 0.9 && p.gamma_32 == 0.8 &&
              p.min_neighbors == 7 && !c.getInputCloud() && c.getKeypointsIndices() && c.getKeypointsIndices()->indices.empty();
    // no cloud, an empty cloud: no keypoints, no device
    Cloud out;
    out.push_back(pcl::PointXYZ());
    c.compute(out);
    ok = ok && out.size() == 0;
    auto cloud = boost::make_shared<Cloud>();
    c.setInputCloud(cloud);
    out.push_back(pcl::PointXYZ());
    c.compute(out);
    ok = ok && out.size() == 0 && c.getKeypointsIndices()->indices.empty();
    // what is not built is refused before a device is asked for
    for (int i = 0; i < 8; ++i) {
        pcl::PointXYZ q;
        q.x = (float) i, q.y = (float) (i * i), q.z = 1.f;
        cloud->push_back(q);
    }
    c.setBorderRadius(0.5);
    out.push_back(pcl::PointXYZ());
    c.compute(out);
    ok = ok && out.size() == 0;
    wave::ISSKeypointParams missing("/nonexistent/iss_keypoints.yaml");  // logs, keeps the defaults
    ok = ok && missing.salient_radius == 0.0 && missing.non_max_radius == 0.0 && missing.gamma_21 == 0.975 &&
         missing.gamma_32 == 0.975 && missing.min_neighbors == 5;
    if (argc > 1) {
        wave::ISSKeypointParams file(argv[1]);
        ok = ok && file.salient_radius == 1.0 && file.non_max_radius == 0.5 && file.gamma_21 == 0.975 && file.gamma_32 == 0.975 &&
             file.min_neighbors == 5;
    }
    std::printf("failed checks: %d\\n", ok ? 0 : 1);
    return ok ? 0 : 1;
}
""")
    exe = str(tmp_path / "iss_cpu")
    build(src, exe)
    r = subprocess.run([exe, YAML], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
