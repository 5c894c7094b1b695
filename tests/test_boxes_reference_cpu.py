"""The checker of the cluster boxes, checked (tests/boxes_reference.py): nothing here needs a device.

  a. the two forms of the checker against each other -- limbs in int64 numpy arrays against Python integers member by
     member -- on the clusters of every (shape, tolerance) tests/test_boxes_gpu.py compares the device on, and on every
     whole cloud as one cluster.
  b. the checker's own boxes (numpy's eigh under the rule's order and signs, obb_from) pass the exact and the tolerance
     checks the device's boxes are held to: the bounds are reachable.
  c. cases with known answers: `holes` (the non-finite rows), `point` (zero eigenvalues, identity axes), `rails` (every
     sum exactly representable: centroid and covariance in closed form), -0 below +0, the range flag."""
import numpy as np
import pytest

import boxes_reference as BR
import cluster_reference as CR
import knn_reference as KR

NAMES = KR.NAMES + sorted(CR.OWN)


def _dtype(wm):
    return wm.BOX_DTYPE


def _same(f, s):
    for key in ("n", "flags"):
        assert np.array_equal(f[key], s[key]), key
    for key in ("aabb_min", "aabb_max"):
        assert np.array_equal(f[key].view(np.uint32), s[key].view(np.uint32)), key
    assert (f["totals"] == s["totals"]).all()
    assert np.array_equal(f["cov"], s["cov"]) and np.array_equal(f["mean"], s["mean"])


@pytest.mark.parametrize("name", NAMES)
def test_fast_form_equals_slow_form(name):
    cloud = CR.shapes()[name]
    for tol in [t for n, t in CR.CASES if n == name]:
        ref = CR.brute_case(name, tol)
        _same(BR.boxes(cloud, ref["offsets"], ref["indices"]), BR.boxes_slow(cloud, ref["offsets"], ref["indices"]))
    one = np.array([0, len(cloud)], np.uint32)
    _same(BR.boxes(cloud, one), BR.boxes_slow(cloud, one))


@pytest.mark.parametrize("name", NAMES)
def test_the_checkers_own_boxes_pass_the_checks(wm, name):
    cloud = CR.shapes()[name]
    lists = [(np.array([0, len(cloud)], np.uint32), None)]
    tol = [t for n, t in CR.CASES if n == name][-1]
    ref = CR.brute_case(name, tol)
    lists.append((ref["offsets"], ref["indices"]))
    for off, idx in lists:
        r = BR.boxes(cloud, off, idx)
        box = BR.fill_obb(BR.as_box_array(r, _dtype(wm)), cloud, off, idx)
        BR.check_exact(r, box, cloud, off, idx)
        assert BR.check_properties(r, box, cloud, off, idx) == int(((r["n"] > 0) & ((r["flags"] & BR.RANGE) == 0)).sum())


def test_holes_point_and_rails():
    S = CR.shapes()
    h = BR.boxes(S["holes"], [0, 3000])
    assert h["n"][0] == 2996 and h["flags"][0] == BR.NONFINITE
    p = BR.boxes(S["point"], [0, 500])
    assert p["n"][0] == 500 and not p["cov"].any() and not p["mu"].any() and not p["totals"].any()
    assert [float(v) for v in BR.centroid_exact(p, 0)] == [1.0, 2.0, 3.0]
    r = BR.boxes(S["rails"], [0, 2048])
    # x = i / 8 for i < 1024 on both rails, y = 0 or 1/4, z = 0: every term and every sum is a dyadic rational
    assert r["a"][0].tolist() == [0.0, 0.0, 0.0] and r["aabb_max"][0].tolist() == [127.875, 0.25, 0.0]
    assert r["mean"][0].tolist() == [1023 / 16, 0.125, 0.0]
    want = np.zeros((3, 3))
    want[0, 0] = (1024 ** 2 - 1) / 12 / 64   # the variance of 0 ... 1023, over 8 squared
    want[1, 1] = 1 / 64
    assert np.array_equal(r["cov"][0], want)
    i = np.arange(1024)
    assert r["totals"][0].tolist() == [int(2 * i.sum()) << 53, 1024 << 54, 0, int(2 * (i * i).sum()) << 50,
                                       int(i.sum()) << 51, 0, 1024 << 52, 0, 0]


def test_small_cases_by_hand(wm):
    c = np.float32([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [4, 5, 6], [2 ** 21, 0, 0], [0, 0, 0], [np.inf, 1, 1]])
    off = [0, 2, 2, 3, 4, 6, 7]
    for r in (BR.boxes(c, off), BR.boxes_slow(c, off)):
        assert r["n"].tolist() == [2, 0, 0, 1, 2, 0]
        assert r["flags"].tolist() == [0, BR.EMPTY, BR.EMPTY | BR.NONFINITE, 0, BR.RANGE, BR.EMPTY | BR.NONFINITE]
        assert np.signbit(r["aabb_min"][0][0]) and not np.signbit(r["aabb_max"][0][0])  # -0 below +0
        assert r["aabb_min"][4].tolist() == [0, 0, 0] and r["aabb_max"][4].tolist() == [2 ** 21, 0, 0]
        assert not r["totals"][4].any() and not r["cov"][4].any()
        assert r["aabb_min"][3].tolist() == r["aabb_max"][3].tolist() == [4, 5, 6] and not r["totals"][3].any()
    center, half = BR.obb_from(np.float32([[0, 0, 0], [2, 0, 0], [1, 4, 0]]), [1, 1, 0], np.eye(3, dtype=np.float32)[[1, 0, 2]])
    assert center.tolist() == [1.0, 2.0, 0.0] and half.tolist() == [2.0, 1.0, 0.0]
    assert BR.key32(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf])).tolist() == sorted(
        BR.key32(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf])).tolist())
    assert wm.BOX_DTYPE.itemsize == 128
