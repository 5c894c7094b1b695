"""The host side that wm_sac_segment and wm_sac_segment_batch share is one header (libwave_amd/csrc/wm_sac_walk.hpp):
PCL's loop as a walk over the hypothesis stream's (flag, count) pairs, and the plane of the refit's nine sums.  Here it
is compiled with g++ under the address and undefined-behaviour sanitizers into a stand-alone program
(tests/cpp_host/sac_walk_host.cpp) and run away from any device.  The stream's pairs come from the checker
(tests/sac_reference.py: samples_block, planes_of, axis_valid, counts_of); the program walks them cut into rounds of 1,
7, 256 and 1024 with the rule R = min(round, max_iterations + 1 - it), and every cut must give the checker's
iterations, skipped, hypotheses, best entry and best count -- the values tests/test_sac_reference_cpu.py pins.

"Plane from sums": the nine sums of a planted plane whose coordinates are small dyadic numbers (so the float64 sums
are exact) must give the checker's float64 plane within the bounds tests/test_sac_gpu.py states."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sac_reference as SR
from test_sac_reference_cpu import TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (1, 7, 256, 1024)
U = 2.0 ** -23
# the cases whose streams are walked: (shape, threshold, max_iterations, model)
WALKS = [("scene", 0.05, 50, SR.PLANE), ("scene", 0.05, 1000, SR.PLANE), ("lattice", 0.5, 1000, SR.PLANE),
         ("dups", 0.5, 1000, SR.PLANE), ("line", 0.5, 1000, SR.PLANE), ("scene", 0.05, 200, SR.PARALLEL)]


def _case_index(name, thr, max_it, model):
    for i, (nm, t, m, extra) in enumerate(SR.CASES):
        if (nm, t, m, extra.get("model", SR.PLANE)) == (name, thr, max_it, model):
            return i
    raise KeyError((name, thr, max_it, model))


def _pairs(P, thr, count, extra):
    """entries 0 ... count - 1 of the stream of P (seed 0) -> flags (0 skipped, 1 valid, 2 axis-invalid), counts"""
    pls, ok = SR.planes_of(P, SR.samples_block(0, 0, count, len(P)))
    valid = ok & SR.axis_valid(pls, extra.get("model", SR.PLANE), extra.get("axis", (0, 0, 1)), extra.get("eps_angle", 0.0))
    cnt = np.zeros(count, np.int64)
    cnt[valid] = SR.counts_of(P, pls[valid], SR.thr_f(thr))
    return np.where(~ok, 0, np.where(valid, 1, 2)), cnt


def _planted():
    """500 points within 3/1024 of z = x / 4 + y / 2, every coordinate a multiple of 1/1024 below 16"""
    rng = np.random.default_rng(77)
    x = rng.integers(-512, 513, 500) / 64.0
    y = rng.integers(-512, 513, 500) / 64.0
    z = x / 4 + y / 2 + rng.integers(-3, 4, 500) / 1024.0
    return np.ascontiguousarray(np.c_[x, y, z], np.float32)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_walk_and_plane_from_sums_on_the_host(tmp_path):
    exe = str(tmp_path / "sac_walk_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "libwave_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp_host", "sac_walk_host.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]

    lines, refs = [], {}
    for name, thr, max_it, model in WALKS:
        i = _case_index(name, thr, max_it, model)
        extra = SR.CASES[i][3]
        ref = SR.case(i, optimize=False)
        P = SR.shapes()[name]
        L = ref["hypotheses"] + max(CUTS)  # (a round may evaluate entries behind the stopping point)
        flags, cnt = _pairs(P, thr, L, extra)
        key = "%s-%g-%d-%d" % (name, thr, max_it, model)
        refs[key] = ref
        lines.append("walk %s %d %d %r %d" % (key, len(P), max_it, 0.99, L))
        lines += ["%d %d" % (f, c) for f, c in zip(flags, cnt)]
        if model == SR.PLANE:
            it, skipped, best, entry = TABLE[(name, thr, max_it)]
            assert (ref["iterations"], ref["skipped"], ref["best_hypothesis"]) == (it, skipped, entry)
    # the planted plane: its sums relative to p0 = the first point, exact in float64
    P = _planted()
    nrm = np.array([-0.25, -0.5, 1.0]) / np.linalg.norm([-0.25, -0.5, 1.0])
    model = np.r_[nrm, 0.0].astype(np.float32)
    assert SR.inliers(P, model, SR.thr_f(1.0)).all()
    D = P.astype(np.float64) - P[0].astype(np.float64)
    sums = [D[:, 0].sum(), D[:, 1].sum(), D[:, 2].sum(), (D[:, 0] * D[:, 0]).sum(), (D[:, 0] * D[:, 1]).sum(),
            (D[:, 0] * D[:, 2]).sum(), (D[:, 1] * D[:, 1]).sum(), (D[:, 1] * D[:, 2]).sum(), (D[:, 2] * D[:, 2]).sum()]
    lines.append("sums " + " ".join(float(v).hex() for v in [len(P), *P[0], *model, *sums]))
    src = tmp_path / "pairs.txt"
    src.write_text("\n".join(lines) + "\n")

    run = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "failed checks: 0" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    seen = set()
    for ln in run.stdout.splitlines():
        tok = ln.split()
        if tok[0] in refs:
            ref = refs[tok[0]]
            cut, it, skipped, hyp, entry, best, rounds = (int(v) for v in tok[1:])
            assert (it, skipped, hyp, entry) == (ref["iterations"], ref["skipped"], ref["hypotheses"], ref["best_hypothesis"]), ln
            assert best == (ref["n_inliers_model"] if entry >= 0 else -1), ln
            assert rounds >= -(-hyp // cut) and (rounds == hyp if cut == 1 else rounds <= hyp), ln
            seen.add((tok[0], cut))
        elif tok[0] == "plane":
            coef = np.array([float.fromhex(v) for v in tok[1:]])
            assert (coef == coef.astype(np.float32)).all()
            f = SR.refit(P, model, 1.0)
            l0, l1, l2 = f["lam"]
            n, d = coef[:3], coef[3]
            assert n @ f["C"] @ n <= l0 * (1 + 1e-9) + 1e-12 * l2
            assert abs(np.linalg.norm(n) - 1) <= 4 * U
            assert abs(d + n @ f["centroid"]) <= 4 * float(np.spacing(np.float32(max(1.0, abs(d)))))
            assert n @ model[:3].astype(np.float64) > 0
            assert l1 >= 100 * l0 > 0 and np.abs(n - f["n"]).max() <= 4 * U
            seen.add("plane")
    assert seen == {(k, c) for k in refs for c in CUTS} | {"plane"}
