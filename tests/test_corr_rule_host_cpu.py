"""The rule of wm_corr_ransac is one header for host and device (libwave_amd/csrc/wm_corr_rule.hpp).  Here it is
compiled with g++ under the address and undefined-behaviour sanitizers into a stand-alone program
(tests/cpp_host/corr_rule_host.cpp) and run away from any device: its own checks on degenerate, duplicate, non-finite
and 1e5-metre-offset samples, the automatic sample distance and the refit from their sums; and a list of samples from
here whose twelve floats must equal, bit for bit, what the library's own build of the same header returns
(wm.corr_hypothesis) -- two compilers, one rule, no fused operation on either side."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import corr_ransac_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _samples():
    rng = np.random.default_rng(21)
    out = []
    for k in range(400):
        off = (0.0, 1.0e3, 1.0e5)[k % 3]
        p = (rng.uniform(-10, 10, (3, 3)) + off).astype(F)
        R = CR.rotation(rng.normal(size=3), rng.uniform(0, math.pi))
        q = ((p.astype(np.float64) - off) @ R.T + off + rng.uniform(-5, 5, 3)).astype(F)
        if k % 7 == 0:
            p[1] = p[0]  # a duplicate
        if k % 11 == 0:
            q[2, 1] = np.nan
        if k % 13 == 0:
            p[2] = p[0] + (p[1] - p[0]) * F(0.5)  # collinear to rounding
        out.append((p, q, float(F(rng.uniform(0, 4))) if k % 2 else 0.0))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_rule_on_the_host_under_the_sanitizers(wm, tmp_path):
    exe = str(tmp_path / "corr_rule_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "libwave_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp_host", "corr_rule_host.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    samples = _samples()
    src = tmp_path / "samples.txt"
    src.write_text("".join("hyp " + " ".join(float(v).hex() for v in [*p.ravel(), *q.ravel(), d]) + "\n" for p, q, d in samples))
    run = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "failed checks: 0" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    rows = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("hyp ")]
    assert len(rows) == len(samples)
    valid = 0
    for (p, q, d), row in zip(samples, rows):
        flag, T = wm.corr_hypothesis(p, q, d)
        got = np.array([float.fromhex(v) for v in row[2:]], F)
        assert int(row[1]) == flag
        assert np.array_equal(got.view(np.uint32), T.ravel().view(np.uint32)), (p, q, d)
        valid += flag
    assert 100 < valid < len(samples)
