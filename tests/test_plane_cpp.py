"""wave::ICPMatcher::setErrorMetric(PointToPlane) (include/wave/matching/icp.hpp), built with g++ against the in-tree
libwave_matching.so (tests/cpp_plane/plane_cases.cpp).  CPU: the header compiles on its own, a default-constructed
matcher reports PointToPoint.  GPU: the reference's fullResNullMatch / nullDisplacement / smallDisplacement fixtures
with the plane metric and estimateInfo() after them; a MultiMatcher<ICPMatcher> queue returns the transforms of
matchers used pair by pair."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "plane_cases")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_plane", "plane_cases.cpp"), "-o", exe, "-L" + LIB, "-lwave_matching",
                        "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k != "WAVE_ICP_ERROR_METRIC"}
    env.update(kw)
    return env


@needs_gxx
def test_icp_header_compiles_standalone(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("#include <wave/matching/icp.hpp>\nint main() { return wave::ICPMatcher::ErrorMetric::PointToPlane == "
                   "wave::ICPMatcher::ErrorMetric::PointToPoint; }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_default_matcher_is_point_to_point(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, ROOT, "defaultMetric"], capture_output=True, text=True, timeout=120, env=_env(HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "cases run: 1, failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


@needs_gxx
@pytest.mark.gpu
def test_reference_fixtures_with_the_plane_metric(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, ROOT, "registrations"], capture_output=True, text=True, timeout=600, env=_env())
    print(r.stdout)
    assert r.returncode == 0 and "cases run: 1, failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]


@needs_gxx
@pytest.mark.gpu
def test_multimatcher_queue_returns_the_same_transforms(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, ROOT, "multiMatcher"], capture_output=True, text=True, timeout=600, env=_env(WAVE_ICP_ERROR_METRIC="plane"))
    print(r.stdout)
    assert r.returncode == 0 and "cases run: 1, failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
