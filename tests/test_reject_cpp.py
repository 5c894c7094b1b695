"""wave::ICPMatcher::setRejector (include/wave/matching/icp.hpp), built with g++ against the in-tree libwave_matching.so
(tests/cpp_reject/reject_cases.cpp).  CPU: the header compiles on its own, a default-constructed matcher reports
Rejector::None and copies carry a setting.  GPU: the reference's smallDisplacement fixture with each rejector and
estimateInfo() after it, an invalid ratio and a device group refused; a MultiMatcher<ICPMatcher> queue under
WAVE_ICP_REJECTOR returns the transforms of matchers used pair by pair."""
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
    exe = str(tmp_path / "reject_cases")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp_reject", "reject_cases.cpp"), "-o", exe, "-L" + LIB, "-lwave_matching",
                        "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WAVE_ICP_ERROR_METRIC", "WAVE_ICP_REJECTOR")}
    env.update(kw)
    return env


@needs_gxx
def test_icp_header_compiles_standalone(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("#include <wave/matching/icp.hpp>\nint main() { return wave::ICPMatcher::Rejector::Trimmed == "
                   "wave::ICPMatcher::Rejector::None; }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_default_matcher_has_no_rejector(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, ROOT, "defaultRejector"], capture_output=True, text=True, timeout=120, env=_env(HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "cases run: 1, failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]


@needs_gxx
@pytest.mark.gpu
def test_small_displacement_fixture_with_each_rejector(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, ROOT, "registrations"], capture_output=True, text=True, timeout=600, env=_env())
    print(r.stdout)
    assert r.returncode == 0 and "cases run: 1, failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]


@needs_gxx
@pytest.mark.gpu
def test_multimatcher_queue_returns_the_same_transforms(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, ROOT, "multiMatcher"], capture_output=True, text=True, timeout=600, env=_env(WAVE_ICP_REJECTOR="trimmed:0.7"))
    print(r.stdout)
    assert r.returncode == 0 and "cases run: 1, failed checks: 0" in r.stdout, r.stdout + r.stderr[-2000:]
