"""The nearest-first visiting order of the grid search's row walks (libwave_amd/csrc/wm_zigzag.hpp), compiled with g++:
the step -> coordinate map must visit every cell of an interval exactly once, outwards from the start cell, and the
distance bound the walks stop on must never exceed the true distance of a cell still to come (a stop that came too early
would lose a neighbour; one that comes late only costs time)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_walk_visits_every_cell_once_outwards_and_its_stop_bound_is_safe(tmp_path):
    exe = str(tmp_path / "zigzag_host")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "libwave_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp_host", "zigzag_host.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 6 * sum(w * 5 for w in range(1, 14))
    for line in lines:
        head, seq, rem = line.split("|")
        lo, c, hi = (int(v) for v in head.split()[:3])
        frac = float.fromhex(head.split()[3])
        seq = [int(v) for v in seq.split()]
        rem = [float.fromhex(v) for v in rem.split()]
        assert seq[0] == c
        assert sorted(seq) == list(range(lo, hi + 1)), line          # every cell, once
        off = [abs(v - c) for v in seq]
        assert off == sorted(off), line                              # outwards
        m = min(c - lo, hi - c)
        assert seq[:2 * m + 1] == [c + ((k + 1) // 2 if k % 2 else -(k // 2)) for k in range(2 * m + 1)], line
        # the query sits at c + frac; its distance along the axis to cell v (the walks' own expression)
        f = c + frac
        dist = [max(v - f, f - (v + 1), 0.0) for v in seq]
        assert rem[0] == 0.0 and rem == sorted(rem), line            # grows: a stop is final
        for k in range(len(seq)):
            assert rem[k] <= min(dist[k:]), (line, k)
        # ... and it is no idle bound: within one cell of the nearest cell left
        for k in range(1, len(seq)):
            assert rem[k] >= min(dist[k:]) - 1.0, (line, k)
