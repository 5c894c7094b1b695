"""tests/fpfh_reference.py against PCL's own formulae, on the CPU: the float32 rule of include/wavematch.h ("feature
descriptors") and a literal float64 restatement of pcl::computePairFeatures / FPFHEstimation's binning give the same
three bins for every pair that is not ambiguous.  A pair is ambiguous when | |a1| - |a2| | < 1e-4 and the two swap
choices give different bins, or when one of its three bin coordinates lies within 1e-4 of an integer; at most 5 % of
the pairs may be (measured on the three clouds: 3.7 / 4.2 / 3.8 % at k = 10, 1.1 / 1.3 / 1.2 % at k = 32).  Also: the reference's second pass and match on hand-made cases, and wm_fpfh_estimate /
wm_feature_match refusing bad arguments before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import fpfh_reference as FR
import knn_reference as KR
import plane_reference as PR

CLOUDS = ["scene", "rings", "scan"]
MAX_AMBIGUOUS = 0.05


def _normals(cloud):
    nrm = PR.normals(cloud, k=10, nbrs=KR.brute(cloud, 11))["normal"]
    return np.ascontiguousarray(nrm, np.float32)


@pytest.mark.parametrize("k", [10, 32])
@pytest.mark.parametrize("name", CLOUDS)
def test_rule_gives_pcl_bins_on_every_unambiguous_pair(name, k):
    cloud = FR.clouds()[name]
    nrm = _normals(cloud)
    idx, d2 = KR.brute(cloud, k)
    p, n_p, q, n_q, live = FR._pairs(cloud, nrm, idx, d2)
    rule = FR.pair_features(p, n_p, q, n_q)
    pcl = FR.pair_features(p, n_p, q, n_q, dtype=np.float64, pcl=True)
    alt = FR.pair_features(p, n_p, q, n_q, dtype=np.float64, pcl=True, swap=~pcl["swap"])
    assert live.sum() >= len(cloud) * (k - 1) * 0.99
    assert np.array_equal(rule["ok"][live], pcl["ok"][live])
    use = live & pcl["ok"]
    close = np.abs(np.abs(pcl["a1"]) - np.abs(pcl["a2"])) < FR.AMBIGUOUS_EPS
    ambiguous = (close & np.any(pcl["bins"] != alt["bins"], axis=-1)) | FR.near_integer(pcl["x1"]) | \
        FR.near_integer(pcl["x2"]) | FR.near_integer(pcl["x3"])
    share = float((ambiguous & use).sum()) / float(use.sum())
    print("%s k=%d: %d pairs, ambiguous %.3f %%" % (name, k, use.sum(), 100 * share))
    clear = use & ~ambiguous
    assert np.array_equal(rule["bins"][clear], pcl["bins"][clear])
    assert np.array_equal(rule["swap"][clear & ~close], pcl["swap"][clear & ~close])
    assert share <= MAX_AMBIGUOUS


def test_hist_incr_cancels_in_the_second_pass():
    """PCL adds 100 / (k - 1) per count; the normalisation to 100 per block removes the factor (to rounding)."""
    cloud = FR.clouds()["scan"][:1500]
    nrm = _normals(cloud)
    idx, d2 = KR.brute(cloud, 10)
    counts, out, _ = FR.fpfh(cloud, nrm, idx, d2)
    w = np.where(d2 != 0, 1.0 / np.where(d2 != 0, d2, 1).astype(np.float64), 0.0)
    pcl = np.einsum("nk,nkb->nb", w, counts[idx].astype(np.float64) * (100.0 / 9.0))
    for f in range(3):
        blk = pcl[:, f * 11:(f + 1) * 11]
        s = blk.sum(axis=1, keepdims=True)
        blk *= np.where(s != 0, 100.0 / np.where(s != 0, s, 1), 0)
    valid = ~np.all(nrm == 0, axis=1)
    assert np.allclose(out[valid], pcl[valid], rtol=1e-4, atol=1e-3)
    sums = out.reshape(-1, 3, 11).astype(np.float64).sum(axis=2)
    assert np.all((np.abs(sums - 100) < 1e-3) | (sums == 0))


def test_pair_rules_by_hand():
    p = np.float32([[0, 0, 0]])
    up = np.float32([[0, 0, 1]])
    # a duplicate, a zero normal and dp parallel to n1 (|v| == 0) are skipped
    assert not FR.pair_features(p, up, p, up)["ok"][0]
    assert not FR.pair_features(p, up, np.float32([[1, 0, 0]]), np.float32([[0, 0, 0]]))["ok"][0]
    assert not FR.pair_features(p, up, np.float32([[0, 0, 2]]), up)["ok"][0]
    # two parallel normals across x: a1 = a2 = 0, no swap, f1 = 0, f2 = 0, f3 = 0 -> the middle bins
    f = FR.pair_features(p, up, np.float32([[1, 0, 0]]), up)
    assert f["ok"][0] and not f["swap"][0] and f["bins"][0].tolist() == [5, 5, 5]
    # |a1| < |a2| swaps
    f = FR.pair_features(p, up, np.float32([[1, 0, 0]]), np.float32([[0.6, 0, 0.8]]))
    assert f["swap"][0] and f["f3"][0] == np.float32(-0.6)


def test_match_reference_by_hand():
    a = np.zeros((4, 33), np.float32)
    b = np.zeros((5, 33), np.float32)
    a[0, 0], a[1, 5], a[3, 32] = 1, 2, 3
    b[0, 5], b[1, 0], b[2, 0], b[4, 32] = 2, 1, 1, 2.5
    idx, d2 = FR.match(a, b)
    assert idx.tolist() == [1, 0, -1, 4] and d2.tolist() == [0, 0, 0, 0.25]  # (duplicates: the lowest index; zero rows: none)
    idx, d2 = FR.match(b, a, reciprocal=True)
    assert idx.tolist() == [1, 0, -1, -1, 3]
    idx, _ = FR.match(a, np.zeros((0, 33), np.float32))
    assert idx.tolist() == [-1] * 4


def test_entry_points_refuse_bad_arguments_without_a_device(wm):
    """wm_fpfh_estimate and wm_feature_match check their arguments before they touch a device."""
    L = wm.lib()
    rows = np.ones((4, 36), np.float32)
    idx = np.zeros(4, np.int32)
    ptr = C.c_void_p(rows.ctypes.data)
    out = C.c_void_p(idx.ctypes.data)
    host = wm.WM_MEM_HOST
    assert L.wm_feature_match(None, ptr, 4, 144, ptr, 4, 144, host, 0, out, None, host, None) == wm.WM_ERR_ARG
    assert L.wm_fpfh_estimate(None, 1, None, None, ptr, None, host, None) == wm.WM_ERR_ARG
    p = wm.fpfh_params()
    assert (p.normal_k, p.feature_k) == (10, 10)
    assert wm.fpfh_params(feature_k=32).feature_k == 32
    with pytest.raises(AttributeError):
        wm.fpfh_params(radius=1.0)
    assert C.sizeof(wm.FpfhParams) == 8 and wm.WM_FEATURE_DIM == 33 and wm.WM_FEATURE_MAX_ROWS == 1 << 20
