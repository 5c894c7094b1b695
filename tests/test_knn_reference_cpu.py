"""The checker of the k-NN stress tests, checked: tests/knn_reference.py's brute force against the oracle's kd-tree on every
stress shape -- two independent statements of "the k nearest by (float32 d2, index)" that must agree to the bit, ties
included, so that either may serve as the expected value on the device -- and the share of points the normals comparison
leaves out, for the reference alone, on exactly the (shape, k) the device test uses."""
import numpy as np
import pytest

import knn_reference as KR
import plane_reference as PR


def test_shapes_are_what_they_claim():
    S = KR.shapes()
    assert sorted(S) == sorted(KR.NAMES)
    for name, c in S.items():
        assert c.dtype == np.float32 and c.ndim == 2 and c.shape[1] == 3 and 500 <= len(c) <= 3400, name
        assert np.isfinite(c).all() == (name != "holes"), name
    assert np.ptp(S["exact_plane"][:, 2]) == 0 and np.ptp(S["line"][:, 1:], axis=0).max() == 0
    assert len(np.unique(S["point"], axis=0)) == 1
    assert len(np.unique(S["dups"], axis=0)) == 1000
    assert np.abs(S["clumps_outliers"]).max() > 100
    bad = np.nonzero(~np.isfinite(S["holes"]).all(1))[0]
    assert bad.tolist() == [0, 17, 1500, len(S["holes"]) - 1]
    # ties that straddle the k-th place: an inner lattice point has 6 neighbours at the pitch, 12 at sqrt 2, 8 at sqrt 3
    _, d2 = KR.brute(S["lattice"], 27)
    inner = d2[:, 26] == np.float32(0.75)
    assert inner.sum() == 13 ** 3
    assert (d2[inner, 1:7] == np.float32(0.25)).all() and (d2[inner, 7:19] == np.float32(0.5)).all()


def test_brute_on_a_case_small_enough_to_read():
    c = np.float32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0], [1, 0, 0]])
    idx, d2 = KR.brute(c, 3)
    assert idx.tolist() == [[0, 1, 4], [1, 4, 0], [-1, -1, -1], [3, 0, 1], [1, 4, 0]]  # equal distances: lowest index first
    assert d2.tolist() == [[0, 1, 1], [0, 0, 1], [0, 0, 0], [0, 4, 5], [0, 0, 1]]
    idx, d2 = KR.brute(c, 5)  # four finite points: the fifth place stays empty
    assert idx[:, 4].tolist() == [-1] * 5 and d2[:, 4].tolist() == [0] * 5 and idx[0].tolist() == [0, 1, 4, 3, -1]


@pytest.mark.parametrize("name", KR.NAMES)
def test_brute_equals_the_oracles_kdtree(oracle, name):
    cloud = KR.shapes()[name]
    finite = np.isfinite(cloud).all(1)
    rows = np.nonzero(finite)[0]
    tree = oracle.KdTree(cloud[finite])
    for k in (3, 10, 20, 32):
        bi, bd = KR.brute(cloud, k)
        oi, od = tree.knn(cloud[finite], k)
        oi = rows[oi].astype(np.int32)  # the tree's indices count the finite points only
        assert np.array_equal(bi[finite], oi), (name, k, int(np.argmax((bi[finite] != oi).any(1))))
        assert np.array_equal(bd[finite].view(np.uint32), od.view(np.uint32)), (name, k)
        assert (bi[~finite] == -1).all() and (bd[~finite] == 0).all()


@pytest.mark.parametrize("name", KR.NORMAL_SHAPES)
def test_the_normals_reference_leaves_out_less_than_its_cap(name):
    """(gap < 1e-3 or a float tie at the k-th place) on at most 1 % of the points: a device test that leaves those out
    cannot hide a failing kernel behind them"""
    cloud = KR.shapes()[name]
    for k in KR.NORMAL_KS:
        ref = PR.normals(cloud, k, nbrs=KR.brute(cloud, k + 1), origin=KR.normal_origin(name))
        share = ((ref["gap"] < 1e-3) | ref["tie"]).mean()
        print("%s k = %d: left out %.3f %%" % (name, k, 100 * share))
        assert share <= KR.NORMAL_CAP, (name, k, share)
        assert ref["valid"].all()


def test_normals_origin_changes_only_the_rounding():
    """about raw coordinates the float64 covariance of utm_plane loses ~(5e4)^2 x 2^-52 ~ 6e-7 of ~0.1: the normals with
    and without the origin agree to ~1e-5 rad, and on a cloud near zero subtracting a whole-number origin changes nothing
    beyond rounding"""
    S = KR.shapes()
    k = 10
    a = PR.normals(S["utm_plane"], k, nbrs=KR.brute(S["utm_plane"], k + 1))
    b = PR.normals(S["utm_plane"], k, nbrs=KR.brute(S["utm_plane"], k + 1), origin=KR.UTM)
    use = b["gap"] >= 1e-3
    assert PR.angle(a["normal"][use], b["normal"][use]).max() < 1e-4
    # near zero a whole-number origin costs nothing: the covariance is about the neighbourhood mean either way
    c = PR.normals(S["noisy_plane"], k, nbrs=KR.brute(S["noisy_plane"], k + 1))
    d = PR.normals(S["noisy_plane"], k, nbrs=KR.brute(S["noisy_plane"], k + 1), origin=[1.0, -2.0, 3.0])
    assert PR.angle(c["normal"], d["normal"]).max() < 1e-9
    assert np.abs(c["curvature"] - d["curvature"]).max() < 1e-12
