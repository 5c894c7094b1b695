"""The saliency step of wm_iss_keypoints is one header for host and device (libwave_amd/csrc/wm_iss_rule.hpp).  Here it
is compiled with g++ under the address and undefined-behaviour sanitizers into a stand-alone program
(tests/cpp_host/iss_rule_host.cpp) and run away from any device: its own checks on zero, huge, negative-definite and
rank-deficient sums; and a list of sums from here whose value must equal, bit for bit, what the library's own build of
the same header returns (wm.iss_third) and what the Python restatement gives (iss_reference.third_from_sums) -- two
compilers and an interpreter, one rule, no fused operation anywhere."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import iss_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v):
    return struct.pack("<d", v)


def _samples():
    rng = np.random.default_rng(31)
    out = []
    for k in range(600):
        n = int(rng.integers(1, 60))
        d = rng.normal(size=(n, 3)) * rng.uniform(0.05, 1.0, 3)
        if k % 5 == 0:
            d[:, 2] *= 1e-3  # nearly planar
        if k % 7 == 0:
            d[:, 1] = d[:, 0]  # rank deficient
        big = 2.0 ** int(rng.integers(10, 34))
        t = np.rint(np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                              d[:, 2] * d[:, 2]], 1) * big).astype(np.int64)
        sums = [int(v) for v in t.sum(0)]
        if k % 11 == 0:
            sums = [-v for v in sums]
        if k % 13 == 0:
            sums = [v << max(61 - max(abs(u).bit_length() for u in sums), 0) for v in sums]  # up to about 2^61
        g = (0.975, 0.975) if k % 3 else (float(rng.uniform(0, 1.2)), float(rng.uniform(0, 1.2)))
        out.append((sums, n, int(rng.integers(-20, 12)), g[0], g[1], int(rng.integers(0, 12))))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_rule_on_the_host_under_the_sanitizers(wm, tmp_path):
    exe = str(tmp_path / "iss_rule_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "libwave_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp_host", "iss_rule_host.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    samples = _samples()
    src = tmp_path / "samples.txt"
    src.write_text("".join("thr %s %d %d %s %s %d\n" % (" ".join(str(v) for v in s), n, x, g21.hex(), g32.hex(), mn)
                           for s, n, x, g21, g32, mn in samples))
    run = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "failed checks: 0" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    rows = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("thr ")]
    assert len(rows) == len(samples)
    positive = 0
    for (s, n, x, g21, g32, mn), row in zip(samples, rows):
        host = float.fromhex(row[1])
        lib = wm.iss_third(s, n, x, gamma_21=g21, gamma_32=g32, min_neighbors=mn)
        ref = IR.third_from_sums(s, n, x, g21, g32, mn)
        assert _bits(host) == _bits(lib) == _bits(ref), (s, n, x, g21, g32, mn, host, lib, ref)
        positive += host > 0
    assert 100 < positive < len(samples)
