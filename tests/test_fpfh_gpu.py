"""wm_fpfh_estimate (libwave_amd/csrc/wm_fpfh.hip) on the GPU against tests/fpfh_reference.py.

First pass: the device's normals and lists (Context.debug_knn) go to the reference; the SPFH counts must EQUAL the
reference's, except at points with a pair whose f1 bin coordinate (float64) lies within 1e-4 of an integer -- atan2f is
the one function of the rule that is not bit-defined.  There the f2 and f3 blocks are still equal, the f1 block has
the same sum and is within L1 distance 2 per such pair; at most 2 % of the points may be such (measured: 0.07-0.68 %,
growing with k).  Second pass: the
reference's weighting of the device's own counts and lists equals fpfh_out bit for bit, at every point.

Zero normals: the device's normal is (0, 0, 0) only where a point's normal_k nearest points all coincide (a clump of
exact duplicates); a collinear clump gets an arbitrary perpendicular from the SVD.  Both are covered: duplicates with
estimated normals, and a collinear clump whose normals the caller zeroes (normals_in)."""
import ctypes as C

import numpy as np
import pytest

import fpfh_reference as FR

pytestmark = pytest.mark.gpu

MAX_RISKY_POINTS = 0.02
LADDER_EDGES = [8, 9, 12, 13, 16, 17, 20, 21, 24, 25]  # knn_ladder's rungs (wm_gicp_dev.hpp) besides 10 / 11


@pytest.fixture(scope="module")
def dev(wm):
    c = wm.Context(0)
    yield c
    c.close()


def run(dev, cloud, k, which=1, normals=None, normal_k=10):
    """-> (result dict, normals, idx, d2) with the cloud as both clouds of the context"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    dev.set_source(cloud)
    dev.set_target(cloud)
    nrm = dev.estimate_normals(which, k=normal_k) if normals is None else np.ascontiguousarray(normals, np.float32)
    res = dev.fpfh(which, normals=nrm, counts=True, feature_k=k)
    assert res["rc"] == 0
    idx, d2 = dev.debug_knn(which, k)
    return res, nrm, idx, d2


def check(dev, cloud, k, which=1, normals=None, normal_k=10, max_risky=1.0):
    res, nrm, idx, d2 = run(dev, cloud, k, which, normals, normal_k)
    got = res["counts"]
    want, risky = FR.spfh(cloud, nrm, idx, d2)
    sure = risky == 0
    assert np.array_equal(got[sure], want[sure])
    assert np.array_equal(got[:, 11:], want[:, 11:])
    g1, w1 = got[~sure, :11].astype(np.int32), want[~sure, :11].astype(np.int32)
    assert np.array_equal(g1.sum(axis=1), w1.sum(axis=1))
    assert np.all(np.abs(g1 - w1).sum(axis=1) <= 2 * risky[~sure])
    share = float((~sure).mean())
    print("k=%d which=%d: f1-risky points %.2f %%" % (k, which, 100 * share))
    assert share <= max_risky
    # the second pass, on the device's own counts and lists: bit for bit
    out = FR.weight(got, idx, d2, cloud, nrm)
    assert np.array_equal(res["fpfh"].view(np.uint32), out.view(np.uint32))
    finite = np.isfinite(np.asarray(cloud)[:, :3]).all(axis=1)
    assert res["n_valid"] == int((finite & np.any(nrm[:, :3] != 0, axis=1)).sum())
    return res, nrm


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("k", [3, 10, 11, 32])
@pytest.mark.parametrize("name", ["scene", "rings", "scan"])
def test_both_passes_on_the_clouds(dev, name, k, which):
    check(dev, FR.clouds()[name], k, which, max_risky=MAX_RISKY_POINTS)


@pytest.mark.parametrize("k", LADDER_EDGES)
def test_every_rung_of_the_list_ladder(dev, k):
    check(dev, FR.clouds()["scan"][:2500], k, which=k % 2, max_risky=MAX_RISKY_POINTS)


@pytest.mark.parametrize("n", [10, 63, 64, 65, 193])
def test_small_clouds(dev, n):
    rng = np.random.default_rng(n)
    cloud = np.float32(rng.uniform(-2, 2, (n, 3)) + [0, 0, 5])
    for which in (0, 1):
        check(dev, cloud, 10, which)  # (n = 10: n == feature_k == normal_k exactly)


def test_exact_duplicates_are_skipped(dev):
    rng = np.random.default_rng(5)
    cloud = np.float32(rng.uniform(-1, 1, (300, 3)) + [0, 0, 4])
    cloud[100:105] = cloud[100]  # five copies: d2 == 0 entries in lists whose normals are not zero
    res, nrm = check(dev, cloud, 10)
    assert np.any(nrm[100:105, :3] != 0) and np.any(res["fpfh"][100] != 0)
    cloud[200:212] = cloud[200]  # twelve: the normal_k = 10 nearest all coincide, the normal is (0, 0, 0), the row zero
    for which in (0, 1):
        res, nrm = check(dev, cloud, 10, which)
        assert not np.any(nrm[200:212, :3]) and not np.any(res["fpfh"][200:212]) and not np.any(res["counts"][200:212])
        assert res["n_valid"] == 300 - 12


def test_zero_normals_are_skipped_as_neighbours(dev):
    rng = np.random.default_rng(6)
    cloud = np.float32(rng.uniform(-1, 1, (400, 3)) + [0, 0, 4])
    cloud[50:70] = np.float32([0.2, 0.1, 4]) + np.float32(np.arange(20)[:, None] * [0.001, 0.002, 0.0005])  # a collinear clump
    dev.set_source(cloud)
    dev.set_target(cloud)
    nrm = dev.estimate_normals(1, k=10)
    nrm[50:70] = 0
    res, _ = check(dev, cloud, 10, normals=nrm)
    assert not np.any(res["fpfh"][50:70]) and not np.any(res["counts"][50:70])
    # a neighbour of the clump counts fewer pairs than its list has entries
    full = res["counts"][:, :11].sum(axis=1)
    outside = np.r_[0:50, 70:400]
    assert full.max() == 9 and np.any(full[outside] < 9)


def test_non_finite_points(dev):
    cloud = FR.clouds()["scan"][:1200].copy()
    cloud[::7, 0] = np.nan
    cloud[5, 2] = np.inf
    for which in (0, 1):
        res, _ = check(dev, cloud, 10, which)
        bad = ~np.isfinite(cloud).all(axis=1)
        assert not np.any(res["fpfh"][bad]) and not np.any(res["counts"][bad]) and np.any(res["fpfh"][~bad])


@pytest.mark.parametrize("which", [0, 1])
def test_given_normals_give_the_bytes_of_estimated_ones(dev, which):
    cloud = FR.clouds()["rings"][:3000]
    dev.set_source(cloud)
    dev.set_target(cloud)
    own = dev.fpfh(which, counts=True, normal_k=12, feature_k=11)
    nrm = dev.estimate_normals(which, k=12)
    given = dev.fpfh(which, normals=nrm, counts=True, feature_k=11)
    assert own["fpfh"].tobytes() == given["fpfh"].tobytes() and own["counts"].tobytes() == given["counts"].tobytes()
    assert own["n_valid"] == given["n_valid"] > 0 and own["spfh_ms"] > 0 and own["weight_ms"] > 0


def test_device_memory(dev):
    import torch
    cloud = FR.clouds()["scan"][:2000]
    dev.set_source(cloud)
    dev.set_target(cloud)
    host = dev.fpfh(1, counts=True)
    out = torch.empty((2000, 33), dtype=torch.float32, device="cuda")
    nrm = torch.from_numpy(dev.estimate_normals(1, k=10)).cuda()
    got = dev.fpfh(1, normals=nrm, counts=True, out=out)
    assert got["fpfh"].cpu().numpy().tobytes() == host["fpfh"].tobytes()
    assert got["counts"].cpu().numpy().tobytes() == host["counts"].tobytes()


def test_quarter_turn_about_z_changes_no_byte(dev):
    """(x, y, z) -> (-y, x, z) is exact in float, and so is every step of the rule under it."""
    cloud = FR.clouds()["scene"][:4000]
    a, nrm, _, _ = run(dev, cloud, 10)
    turn = lambda v: np.ascontiguousarray(np.c_[-v[:, 1], v[:, 0], v[:, 2:]], np.float32)  # noqa: E731
    b, _, _, _ = run(dev, turn(cloud), 10, normals=turn(nrm))
    assert a["counts"].tobytes() == b["counts"].tobytes() and a["fpfh"].tobytes() == b["fpfh"].tobytes()
    assert np.any(a["fpfh"])


def test_errors(wm, dev):
    L = wm.lib()
    out = np.zeros((100, 33), np.float32)
    ptr = C.c_void_p(out.ctypes.data)

    def call(ctx, which=1, **kw):
        p = wm.fpfh_params(**kw)
        return L.wm_fpfh_estimate(ctx._h, which, C.byref(p), None, ptr, None, wm.WM_MEM_HOST, None)

    fresh = wm.Context(0)
    assert call(fresh) == wm.WM_ERR_STATE  # no clouds
    fresh.close()
    cloud = np.float32(np.random.default_rng(2).uniform(-1, 1, (100, 3)))
    cloud[9:] = np.nan  # nine finite points
    dev.set_source(cloud)
    dev.set_target(cloud)
    for which in (0, 1):
        assert call(dev, which, feature_k=10, normal_k=5) == wm.WM_NOT_CONVERGED
        assert call(dev, which, feature_k=5, normal_k=10) == wm.WM_NOT_CONVERGED
        assert call(dev, which, feature_k=9, normal_k=9) == wm.WM_OK
    for k in (2, 33, -1):
        assert call(dev, feature_k=k) == wm.WM_ERR_ARG and call(dev, normal_k=k) == wm.WM_ERR_ARG
    assert call(dev, which=2) == wm.WM_ERR_ARG
    assert L.wm_fpfh_estimate(dev._h, 1, None, None, ptr, None, 7, None) == wm.WM_ERR_ARG
    assert L.wm_fpfh_estimate(dev._h, 1, None, None, None, None, wm.WM_MEM_HOST, None) == wm.WM_ERR_ARG
