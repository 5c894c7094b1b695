"""wm_outlier_filter (libwave_amd/csrc/wm_outlier.hip) on the GPU against tests/outlier_reference.py, on the stress
shapes of knn_reference.py: collapsed grid axes, duplicates, far outliers, exact float ties (the lattice: every
neighbour at exactly the radius), large offsets, non-finite points.

The statistical filter's mean distances are compared bit for bit, its threshold within one float ulp, and its labels
and kept list must EQUAL the checker's: tests/test_outlier_reference_cpu.py shows that on every (shape, mean_k) used here
no point lies within 4 float ulps of the threshold unless every distance is one value (variance exactly 0, nothing
removed), so no summation order can change a label.  The radius filter's counts are compared exactly, with the strict
d2 < r2; the kept list with and without counts_out, so that the variant that stops at min_neighbors is covered."""
import ctypes as C

import numpy as np
import pytest

import knn_reference as KR
import outlier_reference as OR

pytestmark = pytest.mark.gpu

IP = C.POINTER(C.c_int32)


def _stat(ctx, cloud, mean_k, **kw):
    return ctx.outlier_filter(cloud, method=0, mean_k=mean_k, stddev_mult=OR.STDDEV_MULT, **kw)


def _rad(ctx, cloud, r, **kw):
    return ctx.outlier_filter(cloud, method=1, radius=r, min_neighbors=OR.MIN_NEIGHBORS, **kw)


def _complement(wm, ctx, cloud, got, finite, **params):
    """negative = 1 returns exactly the finite points the positive call did not"""
    neg = ctx.outlier_filter(cloud, negative=1, **params)
    assert neg["rc"] == wm.WM_OK
    both = np.r_[got["indices"], neg["indices"]]
    assert np.array_equal(np.sort(both), np.nonzero(finite)[0]), "kept and removed do not partition the finite points"
    assert (np.diff(neg["indices"]) > 0).all()
    assert np.array_equal(neg["labels"], got["labels"])
    assert (neg["n_inliers"], neg["n_outliers"]) == (got["n_inliers"], got["n_outliers"])


# ------------------------------------------------------------------ the statistical filter
@pytest.mark.parametrize("name", KR.NAMES)
def test_statistical_equals_the_checker(wm, ctx, name):
    cloud = KR.shapes()[name]
    for mean_k in OR.MEAN_KS:
        ref = OR.statistical(cloud, mean_k, OR.STDDEV_MULT)
        got = _stat(ctx, cloud, mean_k)
        what = "%s mean_k %d" % (name, mean_k)
        bad = got["mean_dist"].view(np.uint32) != ref["dist"].view(np.uint32)
        ulps = np.abs(got["mean_dist"].view(np.int32).astype(np.int64) - ref["dist"].view(np.int32).astype(np.int64)).max()
        print("%s: %d distances differ (max %d ulps); threshold %.17g want %.17g (float ulp %.3g); removed %d want %d; fence %d"
              % (what, bad.sum(), ulps, got["threshold"], ref["threshold"], OR.ulp32(ref["threshold"]), got["n_outliers"],
                 (ref["labels"] == OR.OUTLIER).sum(), len(ref["fence"])))
        assert got["rc"] == wm.WM_OK, what
        assert not bad.any(), "%s: first at point %d" % (what, int(np.argmax(bad)))
        assert abs(got["threshold"] - ref["threshold"]) <= OR.ulp32(ref["threshold"]), what
        assert abs(got["mean"] - ref["mean"]) <= OR.ulp32(ref["mean"]) and abs(got["stddev"] - ref["stddev"]) <= OR.ulp32(ref["threshold"])
        assert len(ref["fence"]) == 0 or ref["var"] == 0.0  # (asserted on the CPU for every case; here for the record)
        assert np.array_equal(got["labels"], ref["labels"]), what
        assert np.array_equal(got["indices"], ref["kept"]) and got["indices"].dtype == np.int32, what
        assert got["n_finite"] == ref["n_finite"] and got["n_inliers"] == len(ref["kept"])
        assert got["n_outliers"] == ref["n_finite"] - len(ref["kept"])
        _complement(wm, ctx, cloud, got, ref["finite"], method=0, mean_k=mean_k, stddev_mult=OR.STDDEV_MULT)
        if name == "holes":
            holes = [0, 17, 1500, len(cloud) - 1]
            assert got["n_finite"] == 2996
            assert (got["labels"][holes] == wm.WM_OUTLIER_NONE).all() and (got["mean_dist"][holes] == 0).all()
            assert not np.isin(holes, got["indices"]).any()
        if name == "clumps_outliers":
            far = np.nonzero(np.abs(cloud).max(1) > 20)[0]
            assert len(far) == 12 and np.array_equal(np.nonzero(got["labels"] == wm.WM_OUTLIER_OUTLIER)[0], far)


def test_a_nan_threshold_removes_nothing(wm, ctx):
    """dist > NaN is false for every point, as in PCL's comparison"""
    cloud = np.float32([[0, 0, 0], [1, 0, 0], [5, 0, 0], [5, 1, 0]])
    got = ctx.outlier_filter(cloud, method=0, mean_k=1, stddev_mult=float("nan"))
    assert got["rc"] == wm.WM_OK and np.isnan(got["threshold"])
    assert got["indices"].tolist() == [0, 1, 2, 3] and (got["labels"] == wm.WM_OUTLIER_INLIER).all()


# ------------------------------------------------------------------ the radius filter
@pytest.mark.parametrize("name", KR.NAMES)
def test_radius_equals_the_checker(wm, ctx, name):
    cloud = KR.shapes()[name]
    for r in OR.RADII:
        ref = OR.radius(cloud, r, OR.MIN_NEIGHBORS)
        got = _rad(ctx, cloud, r)
        quick = _rad(ctx, cloud, r, counts=False)  # a point's search may stop at min_neighbors
        what = "%s radius %g" % (name, r)
        bad = got["counts"] != ref["counts"]
        print("%s: %d counts differ; kept %d want %d (without counts_out %d)" % (what, bad.sum(), len(got["indices"]),
                                                                                len(ref["kept"]), len(quick["indices"])))
        assert got["rc"] == wm.WM_OK and quick["rc"] == wm.WM_OK, what
        assert not bad.any(), "%s: first at point %d: got %d want %d" % (
            what, int(np.argmax(bad)), got["counts"][np.argmax(bad)], ref["counts"][np.argmax(bad)])
        assert np.array_equal(got["labels"], ref["labels"]) and np.array_equal(got["indices"], ref["kept"]), what
        assert quick["counts"] is None and np.array_equal(quick["labels"], ref["labels"]), what
        assert np.array_equal(quick["indices"], ref["kept"]), what
        assert got["n_finite"] == ref["n_finite"] and got["n_inliers"] == len(ref["kept"])
        assert (got["mean"], got["stddev"], got["threshold"]) == (0.0, 0.0, 0.0)
        _complement(wm, ctx, cloud, got, ref["finite"], method=1, radius=r, min_neighbors=OR.MIN_NEIGHBORS)
        _complement(wm, ctx, cloud, quick, ref["finite"], method=1, radius=r, min_neighbors=OR.MIN_NEIGHBORS, counts=False)
        if name == "holes":
            holes = [0, 17, 1500, len(cloud) - 1]
            assert got["n_finite"] == 2996 and (got["counts"][holes] == -1).all()
            assert (got["labels"][holes] == wm.WM_OUTLIER_NONE).all() and not np.isin(holes, got["indices"]).any()
        if name == "lattice" and r == 0.5:  # every neighbour at exactly d2 == r2: strict, so nobody has one
            assert (got["counts"] == 0).all() and len(got["indices"]) == 0 and got["n_outliers"] == len(cloud)


@pytest.mark.parametrize("name", ["scene", "lattice", "clumps_outliers", "utm"])
def test_the_cell_rule_changes_no_count(wm, ctx, name):
    """option outlier_cell_div: cells of 2 radii (a box of 2 x 2 rows), the default half radius, an eighth (18 x 18 rows)"""
    cloud = KR.shapes()[name]
    try:
        for div in (0.5, 2.0, 8.0):
            ctx.set_option("outlier_cell_div", div)
            for r in OR.RADII:
                ref = OR.radius(cloud, r, OR.MIN_NEIGHBORS)
                got = _rad(ctx, cloud, r)
                assert np.array_equal(got["counts"], ref["counts"]), (name, div, r)
                assert np.array_equal(_rad(ctx, cloud, r, counts=False)["indices"], ref["kept"]), (name, div, r)
    finally:
        ctx.set_option("outlier_cell_div", 2.0)


def test_min_neighbors_zero_and_a_radius_that_rounds_to_zero(wm, ctx):
    cloud = KR.shapes()["dups"]
    got = ctx.outlier_filter(cloud, method=1, radius=1e-30, min_neighbors=1)  # r2 = 0 in float: d2 < 0 never holds
    assert (got["counts"] == 0).all() and len(got["indices"]) == 0
    got = ctx.outlier_filter(cloud, method=1, radius=1e-30, min_neighbors=0)
    assert len(got["indices"]) == len(cloud)
    got = ctx.outlier_filter(cloud, method=1, radius=1e-6, min_neighbors=2)  # only the duplicates: two others each
    assert (got["counts"] == 2).all() and len(got["indices"]) == len(cloud)
    got = ctx.outlier_filter(cloud, method=1, radius=1e6, min_neighbors=len(cloud) - 1)  # everything is inside
    assert (got["counts"] == len(cloud) - 1).all() and len(got["indices"]) == len(cloud)


# ------------------------------------------------------------------ both filters: memory, strides, cap, sizes
@pytest.mark.parametrize("params", [dict(method=0, mean_k=8, stddev_mult=1.0), dict(method=1, radius=2.0, min_neighbors=5)])
def test_host_and_device_memory_and_both_strides_give_the_same_bytes(wm, ctx, params):
    import torch
    cloud = KR.shapes()["holes"]
    key = "mean_dist" if params["method"] == 0 else "counts"
    first = ctx.outlier_filter(cloud, **params)
    assert len(first["indices"]) > 0 and first["n_outliers"] > 0
    c4 = np.c_[cloud, np.full(len(cloud), 7.0, np.float32)].astype(np.float32)
    for host in (c4, cloud):
        for arr in (host, torch.from_numpy(host.copy()).cuda()):
            got = ctx.outlier_filter(arr, **params)
            if not isinstance(arr, np.ndarray):
                assert got["indices"].is_cuda and got["labels"].is_cuda and got[key].is_cuda
                got = dict(got, indices=got["indices"].cpu().numpy(), labels=got["labels"].cpu().numpy(), **{key: got[key].cpu().numpy()})
            for k in ("indices", "labels", key):
                assert got[k].tobytes() == first[k].tobytes(), (k, host.shape, type(arr))
            assert (got["threshold"], got["n_finite"], got["n_inliers"]) == (first["threshold"], first["n_finite"], first["n_inliers"])


@pytest.mark.parametrize("params", [dict(method=0, mean_k=8, stddev_mult=1.0), dict(method=1, radius=2.0, min_neighbors=5)])
def test_cap_one_short_is_an_argument_error_with_the_true_count(wm, ctx, params):
    cloud = KR.shapes()["scene"]
    full = ctx.outlier_filter(cloud, **params)
    kept = len(full["indices"])
    assert 1 < kept < len(cloud)
    p = wm.outlier_params(params)
    out = np.full(kept, -7, np.int32)
    m = C.c_size_t(0)
    rc = wm.lib().wm_outlier_filter(ctx._h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, wm.WM_MEM_HOST, C.byref(p),
                                    C.c_void_p(out.ctypes.data), kept - 1, wm.WM_MEM_HOST, C.byref(m), None, None, None, None)
    assert rc == wm.WM_ERR_ARG and m.value == kept
    assert np.array_equal(out[:kept - 1], full["indices"][:kept - 1]) and out[kept - 1] == -7
    import torch
    dev = torch.from_numpy(cloud.copy()).cuda()
    dout = torch.full((kept,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = wm.lib().wm_outlier_filter(ctx._h, C.c_void_p(dev.data_ptr()), len(cloud), 12, wm.WM_MEM_DEVICE, C.byref(p),
                                    C.c_void_p(dout.data_ptr()), kept - 1, wm.WM_MEM_DEVICE, C.byref(m), None, None, None, None)
    assert rc == wm.WM_ERR_ARG and m.value == kept
    assert np.array_equal(dout.cpu().numpy(), np.r_[full["indices"][:kept - 1], np.int32(-7)])


@pytest.mark.parametrize("mean_k", [1, 8, 31])
def test_a_cloud_of_mean_k_finite_points_is_not_converged(wm, ctx, mean_k):
    cloud = np.random.default_rng(mean_k).uniform(-2, 2, (mean_k, 3)).astype(np.float32)
    holed = np.r_[cloud, np.float32([[np.nan, 0, 0]])]  # (a non-finite point does not count)
    for c in (cloud, holed):
        got = ctx.outlier_filter(c, method=0, mean_k=mean_k, stddev_mult=1.0)
        assert got["rc"] == wm.WM_NOT_CONVERGED and len(got["indices"]) == 0
    one_more = np.r_[cloud, np.float32([[0.5, 0.5, 0.5]])]
    got = ctx.outlier_filter(one_more, method=0, mean_k=mean_k, stddev_mult=1.0)
    ref = OR.statistical(one_more, mean_k, 1.0)
    assert got["rc"] == wm.WM_OK and np.array_equal(got["mean_dist"].view(np.uint32), ref["dist"].view(np.uint32))
    assert np.array_equal(got["indices"], ref["kept"])


@pytest.mark.parametrize("method", [0, 1])
def test_empty_and_all_nan_clouds_are_ok_with_no_points(wm, ctx, method):
    params = dict(method=method, mean_k=8, stddev_mult=1.0, radius=0.5, min_neighbors=5)
    got = ctx.outlier_filter(np.zeros((0, 3), np.float32), **params)
    assert got["rc"] == wm.WM_OK and len(got["indices"]) == 0 and got["n_finite"] == 0
    nans = np.full((100, 3), np.nan, np.float32)
    nans[::3, 1] = np.inf
    for negative in (0, 1):
        got = ctx.outlier_filter(nans, negative=negative, **params)
        assert got["rc"] == wm.WM_OK and len(got["indices"]) == 0 and got["n_finite"] == 0
        assert (got["labels"] == wm.WM_OUTLIER_NONE).all() and len(got["labels"]) == 100
        extra = got["mean_dist"] if method == 0 else got["counts"]
        assert (extra == (0 if method == 0 else -1)).all()


# ------------------------------------------------------------------ one size above the 256k sort switch
def test_large_scene_against_the_kdtree(wm, ctx, oracle):
    cloud, ref = OR.big_case(oracle)
    assert len(ref["fence"]) == 0  # before anything is compared: no label hangs on the rounding of a sum
    got = _stat(ctx, cloud, OR.BIG_MEAN_K)
    bad = got["mean_dist"].view(np.uint32) != ref["dist"].view(np.uint32)
    print("n %d: %d distances differ; threshold %.17g want %.17g; removed %d want %d; %.2f ms on the device"
          % (len(cloud), bad.sum(), got["threshold"], ref["threshold"], got["n_outliers"], (ref["labels"] == OR.OUTLIER).sum(),
             got["kernel_ms"]))
    assert got["rc"] == wm.WM_OK and not bad.any()
    assert abs(got["threshold"] - ref["threshold"]) <= OR.ulp32(ref["threshold"])
    assert np.array_equal(got["indices"], ref["kept"]) and np.array_equal(got["labels"], ref["labels"])


# ------------------------------------------------------------------ the context's registration state
def test_registration_state_is_not_touched(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    third = KR.shapes()["clumps_outliers"]
    runs = []
    for with_filters in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0)
            knn_a = c.debug_knn(1, 10)
            if with_filters:
                assert len(_stat(c, third, 8)["indices"]) == 3000
                assert _rad(c, third, 0.5)["rc"] == wm.WM_OK
                assert _rad(c, third, 2.0, counts=False)["rc"] == wm.WM_OK
            knn_b = c.debug_knn(1, 10)
            b = c.icp_align(max_corr=3.0)
            assert knn_a[0].tobytes() == knn_b[0].tobytes() and knn_a[1].tobytes() == knn_b[1].tobytes()
            assert c.sizes() == (len(ref_cloud), len(tgt_cloud))
            runs.append((a, b))
        finally:
            c.close()
    (a1, b1), (a2, b2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]
