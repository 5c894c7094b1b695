"""wm_normal_from_sums -- the step of wm_normals_radius from a point's nine integer sums to its record, on the host (no
GPU; libwave_amd/csrc/wm_normal_rule.hpp, the text a lane of k_nr_finish and of k_normals runs) -- against the numpy
finish of tests/fpfh_radius_reference.py on the same sums, and against PCL's arithmetic in float64 (double sums about
the neighbourhood's mean).  svd3 is not restated in Python, so the bars are the ones the k form's normals are held to
(plane_reference.check_normals): unit length, 1e-6 rad, 1e-6 in curvature, turned towards the origin, on every point
whose normal the data determines (eigen-gap >= 1e-3).

The share of points with a smaller gap, measured with the reference alone (numpy's eigenvalues; the code under test has
no part in it), at the normal radius of 3 / 5 median spacings: scene 0.45 / 0.00 %, rings 0.93 / 1.10 %, scan 5.60 /
5.80 %; at the feature radius of 6 / 10: scene 0.00 / 0.00 %, rings 1.52 / 1.27 %, scan 4.72 / 2.05 %.  On the scan the
points of a small ball are those of one ring, a line.  The cap is 10 %, about twice the largest of these."""
import ctypes as C

import numpy as np
import pytest

import fpfh_radius_reference as RR
import fpfh_reference as FR
import plane_reference as PR

CLOUDS = ["scene", "rings", "scan"]
MAX_UNDETERMINED = 0.10


def _host(wm, cloud, s):
    return np.stack([wm.normal_from_sums(s["sums"][i], max(int(s["counts"][i]), 0), s["x"], np.nan_to_num(cloud[i]))
                     for i in range(len(cloud))])


@pytest.mark.parametrize("mult", RR.RADII)
@pytest.mark.parametrize("which", ["normal", "feature"])
@pytest.mark.parametrize("name", CLOUDS)
def test_host_finish_against_numpy_and_pcl(wm, name, which, mult):
    cloud = FR.clouds()[name]
    radius = RR.radii(name, mult)[0 if which == "normal" else 1]
    cap = MAX_UNDETERMINED
    _, s, ref = RR.normals(cloud, radius)
    got = _host(wm, cloud, s)
    what = "%s %s radius %d x" % (name, which, mult)
    assert ref["valid"].mean() > 0.6
    PR.check_normals(got, cloud, 0, what + " (numpy finish)", ref=ref, cap=cap)
    assert np.all(got[~ref["valid"]] == 0)  # n_s < 3, or every neighbour on the point itself
    assert np.all(np.isfinite(got))
    PR.check_normals(got, cloud, 0, what + " (PCL literal)", ref=RR.pcl_normals_literal(cloud, radius), cap=cap)


def test_edges_of_the_step(wm):
    u = 1 << 36
    p = np.float32([0, 0, 5])
    # x = 0: quanta 2^-36.  Four neighbours (the point and three at (+-1, 0, 0) / (0, 1, 0) scaled): a plane z = 0
    sums = [0, u // 2, 0, u // 2, 0, 0, u // 4, 0, 0]  # mean (0, 1/8, 0); xx = 1/8, yy = 1/16 - 1/64
    out = wm.normal_from_sums(sums, 4, 0, p)
    assert np.array_equal(out, np.float32([0, 0, -1, 0]))          # towards the origin from (0, 0, 5)
    assert np.array_equal(wm.normal_from_sums(sums, 4, 0, -p), np.float32([0, 0, 1, 0]))
    assert np.all(wm.normal_from_sums(sums, 2, 0, p) == 0)          # n_s < 3 (PCL: NaN)
    assert np.all(wm.normal_from_sums([0] * 9, 5, 0, p) == 0)       # five coincident points: the largest value is 0
    # x = 3 (e = 2) and x = -3 (e = -1): the same neighbourhood scaled by 2 and by 1 / 4 in length
    for x, e in ((2, 1), (-4, -2)):
        scaled = [v for v in sums]  # (the integers are the same: the quanta carry the scale)
        assert RR.half_exponent(x) == e
        assert np.array_equal(wm.normal_from_sums(scaled, 4, x, p), np.float32([0, 0, -1, 0]))
    L = wm.lib()
    s = (C.c_int64 * 9)()
    pt = (C.c_float * 3)()
    o = (C.c_float * 4)(5, 5, 5, 5)
    assert L.wm_normal_from_sums(None, 4, 0, pt, o) == wm.WM_ERR_ARG
    assert L.wm_normal_from_sums(s, 4, 0, None, o) == wm.WM_ERR_ARG
    assert L.wm_normal_from_sums(s, 4, 0, pt, None) == wm.WM_ERR_ARG
    assert L.wm_normal_from_sums(s, -1, 0, pt, o) == wm.WM_ERR_ARG
    assert L.wm_normal_from_sums(s, 4, 129, pt, o) == wm.WM_ERR_ARG
    assert L.wm_normal_from_sums(s, 4, -126, pt, o) == wm.WM_ERR_ARG
    assert list(o) == [5, 5, 5, 5]
    assert L.wm_normal_from_sums(s, 4, 128, pt, o) == wm.WM_OK and list(o) == [0, 0, 0, 0]
