"""The ICP loop's scalar side is one header (libwave_amd/csrc/wm_icp_ctl.hpp): the step record every solve kernel packs
for the host that runs ahead of it, and the policy that picks an iteration's search kernel from those records.  Here it
is compiled with g++ and run away from any device: the record's round trip and bit layout, the done word, and the
certificate policy's rules one by one (tests/cpp_host/icp_ctl_host.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_step_record_and_certificate_policy_on_the_host(tmp_path):
    exe = str(tmp_path / "icp_ctl_host")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "libwave_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp_host", "icp_ctl_host.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "failed checks: 0" in run.stdout, run.stdout[-3000:] + run.stderr[-1000:]
