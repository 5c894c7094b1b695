"""wm_outlier_filter_batch (libwave_amd/csrc/wm_outlier.hip) on the GPU: every scan of a batch must EQUAL what
wm_outlier_filter gives for that scan alone -- status, kept indices, labels, mean distances or counts, the counters, and
mean, stddev and threshold compared with == on the doubles.  No tolerance anywhere.  On the shapes of knn_reference.py
the labels and kept lists are also held to tests/outlier_reference.py directly (its fence is empty for these shapes:
tests/test_outlier_reference_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import knn_reference as KR
import outlier_reference as OR

pytestmark = pytest.mark.gpu

STAT8 = dict(method=0, mean_k=8, stddev_mult=OR.STDDEV_MULT)
RAD2 = dict(method=1, radius=2.0, min_neighbors=OR.MIN_NEIGHBORS)


def _np(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def _same_scan(wm, got, one, what):
    """one scan of a batch against the single call's dict"""
    assert got["rc"] == one["rc"], what
    assert _np(got["indices"]).tobytes() == _np(one["indices"]).tobytes(), what
    for key in ("labels", "mean_dist", "counts"):
        a, b = _np(got[key]), _np(one[key])
        assert (a is None) == (b is None), (what, key)
        if a is not None:
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, key)
    for key in ("n_finite", "n_inliers", "n_outliers"):
        assert got[key] == one[key], (what, key, got[key], one[key])
    for key in ("mean", "stddev", "threshold"):  # the bits: NaN == NaN here, 0.0 != -0.0
        assert np.float64(got[key]).tobytes() == np.float64(one[key]).tobytes(), (what, key, got[key], one[key])


def _against_singles(wm, ctx, clouds, what="", **params):
    """-> (the batch's dicts, the single calls' dicts), every scan compared"""
    batch = ctx.outlier_filter_batch(clouds, **params)
    assert len(batch) == len(clouds)
    singles = [ctx.outlier_filter(c, **params) for c in clouds]
    for k, (got, one) in enumerate(zip(batch, singles)):
        _same_scan(wm, got, one, "%s scan %d" % (what, k))
    return batch, singles


_REF = {}


def _ref(kind, name, arg, negative):
    """the checker's result, computed once per case and shared"""
    key = (kind, name, arg, negative)
    if key not in _REF:
        cloud = KR.shapes()[name]
        _REF[key] = (OR.statistical(cloud, arg, OR.STDDEV_MULT, negative=bool(negative)) if kind == "stat" else
                     OR.radius(cloud, arg, OR.MIN_NEIGHBORS, negative=bool(negative)))
    return _REF[key]


# ------------------------------------------------------------------ 1. every shape in one batch
@pytest.mark.parametrize("mean_k", OR.MEAN_KS)
def test_all_shapes_statistical(wm, ctx, mean_k):
    clouds = [KR.shapes()[name] for name in KR.NAMES]
    for negative in (0, 1):
        batch, _ = _against_singles(wm, ctx, clouds, "mean_k %d negative %d" % (mean_k, negative), method=0, mean_k=mean_k,
                                    stddev_mult=OR.STDDEV_MULT, negative=negative)
        for name, got in zip(KR.NAMES, batch):
            ref = _ref("stat", name, mean_k, negative)
            assert len(ref["fence"]) == 0 or ref["var"] == 0.0
            assert got["rc"] == wm.WM_OK and np.array_equal(got["labels"], ref["labels"]), (name, mean_k)
            assert np.array_equal(got["indices"], ref["kept"]) and got["indices"].dtype == np.int32, (name, mean_k)
            assert got["mean_dist"].view(np.uint32).tobytes() == ref["dist"].view(np.uint32).tobytes(), (name, mean_k)


@pytest.mark.parametrize("r", OR.RADII)
def test_all_shapes_radius(wm, ctx, r):
    clouds = [KR.shapes()[name] for name in KR.NAMES]
    for negative in (0, 1):
        for counts in (True, False):
            batch, _ = _against_singles(wm, ctx, clouds, "radius %g negative %d counts %d" % (r, negative, counts), method=1,
                                        radius=r, min_neighbors=OR.MIN_NEIGHBORS, negative=negative, counts=counts)
            for name, got in zip(KR.NAMES, batch):
                ref = _ref("rad", name, r, negative)
                assert got["rc"] == wm.WM_OK and np.array_equal(got["labels"], ref["labels"]), (name, r)
                assert np.array_equal(got["indices"], ref["kept"]), (name, r)
                if counts:
                    assert np.array_equal(got["counts"], ref["counts"]), (name, r)
                else:
                    assert got["counts"] is None


# ------------------------------------------------------------------ 2. scans do not leak into each other
@pytest.mark.parametrize("params", [STAT8, dict(method=1, radius=0.5, min_neighbors=OR.MIN_NEIGHBORS)])
def test_copies_in_the_same_space_are_filtered_apart(wm, ctx, params):
    scene = KR.shapes()["scene"]
    batch, singles = _against_singles(wm, ctx, [scene.copy() for _ in range(5)], "five copies", **params)
    assert 0 < len(singles[0]["indices"]) < len(scene)
    for got in batch[1:]:
        _same_scan(wm, got, batch[0], "copy against copy")


def test_a_copy_shifted_by_the_radius_adds_no_neighbour(wm, ctx):
    r = 0.5
    shape = KR.shapes()["lattice"]  # (every neighbour at exactly the radius: the shifted copy sits ON the lattice)
    shifted = shape + np.float32([r, 0, 0])
    batch, singles = _against_singles(wm, ctx, [shape, shifted], "shifted", method=1, radius=r, min_neighbors=1)
    union = OR.radius_counts(np.r_[shape, shifted], r)[0]
    assert not np.array_equal(union[:len(shape)], singles[0]["counts"])  # (the union would count the copy's points)
    assert np.array_equal(batch[0]["counts"], singles[0]["counts"])
    scene = KR.shapes()["scene"]
    _against_singles(wm, ctx, [scene, scene + np.float32([2.0, 0, 0])], "shifted scene", **RAD2)


# ------------------------------------------------------------------ 3. scan boundaries
def _boundary_scans():
    scene, clumps = KR.shapes()["scene"], KR.shapes()["clumps_outliers"]
    nans = np.full((40, 3), np.nan, np.float32)
    nans[::3, 1] = np.inf
    return [scene[:0], scene[5:6], nans, scene[100:163], clumps[:64], scene[200:265], scene[:3000], clumps[:0],
            clumps[1000:1129], scene[7:9]]


@pytest.mark.parametrize("mean_k", [8, 1])
def test_scan_boundaries_statistical(wm, ctx, mean_k):
    scans = _boundary_scans()
    assert [len(s) for s in scans] == [0, 1, 40, 63, 64, 65, 3000, 0, 129, 2]
    short = {1: [1], 8: [1, 2]}[mean_k]
    for order in (scans, scans[::-1], scans + scans):
        params = dict(method=0, mean_k=mean_k, stddev_mult=OR.STDDEV_MULT)
        batch, _ = _against_singles(wm, ctx, order, "boundaries mean_k %d" % mean_k, **params)
        for s, got in zip(order, batch):
            want = wm.WM_NOT_CONVERGED if len(s) in short else wm.WM_OK
            assert got["rc"] == want, (len(s), got["rc"])
            if want != wm.WM_OK:
                assert len(got["indices"]) == 0 and got["n_finite"] == len(s) and got["n_inliers"] == 0 and got["threshold"] == 0.0
        assert sum(len(g["indices"]) for g in batch) > 0
        again = ctx.outlier_filter_batch(order, **params)
        for a, b in zip(batch, again):
            _same_scan(wm, a, b, "a repeated call")


def test_scan_boundaries_radius(wm, ctx):
    scans = _boundary_scans()
    for order in (scans, scans[::-1], scans + scans):
        for counts in (True, False):
            batch, _ = _against_singles(wm, ctx, order, "boundaries radius", counts=counts, **RAD2)
            assert all(g["rc"] == wm.WM_OK for g in batch)
            again = ctx.outlier_filter_batch(order, counts=counts, **RAD2)
            for a, b in zip(batch, again):
                _same_scan(wm, a, b, "a repeated call")
    nan_scan = ctx.outlier_filter_batch(scans, **RAD2)[2]
    assert (nan_scan["labels"] == wm.WM_OUTLIER_NONE).all() and (nan_scan["counts"] == -1).all()


# ------------------------------------------------------------------ 4. the moment tree beyond one pass
def test_a_scan_whose_moment_threads_take_a_second_point(wm, ctx):
    """more than 1024 * 256 points: a thread of the moment kernel takes two, the tree's rows are capped"""
    from libwave_amd import synth
    big = synth.scene(300000, seed=11)
    small_a, small_b = KR.shapes()["scene"][:100], KR.shapes()["clumps_outliers"][:100]
    assert len(big) > 1024 * 256
    batch, singles = _against_singles(wm, ctx, [small_a, big, small_b], "300k between two small scans", **STAT8)
    assert singles[1]["n_outliers"] > 0 and singles[1]["stddev"] > 0
    print("300k: batch %.2f ms on the device, the big scan alone %.2f ms" % (batch[1]["kernel_ms"], singles[1]["kernel_ms"]))


# ------------------------------------------------------------------ 5. memory, strides, points
@pytest.mark.parametrize("params", [STAT8, RAD2])
def test_host_and_device_memory_and_both_strides_give_the_same_bytes(wm, ctx, params):
    import torch
    names = ["holes", "scene", "utm"]
    clouds = [KR.shapes()[n] for n in names] + [np.zeros((0, 3), np.float32)]
    first = ctx.outlier_filter_batch(clouds, points=True, **params)
    assert len(first[0]["indices"]) > 0 and first[0]["n_outliers"] > 0
    for stride in (12, 16):
        host = [c if stride == 12 else np.c_[c, np.full(len(c), 7.0, np.float32)].astype(np.float32) for c in clouds]
        for dev in (False, True):
            arrs = [torch.from_numpy(h.copy()).cuda() for h in host] if dev else host
            got = ctx.outlier_filter_batch(arrs, points=True, **params)
            for k, (g, f, c) in enumerate(zip(got, first, clouds)):
                if dev:
                    assert g["indices"].is_cuda and g["labels"].is_cuda and g["points"].is_cuda
                _same_scan(wm, g, f, "stride %d device %d scan %d" % (stride, dev, k))
                pts = _np(g["points"])
                assert pts.shape == (len(f["indices"]), stride // 4)
                assert pts[:, :3].tobytes() == c[_np(f["indices"])].tobytes()  # bit for bit
                assert not pts[:, 3:].view(np.uint32).any()  # the bytes behind z are zero


def test_device_points_go_into_the_cluster_batch_as_they_are(wm, ctx):
    import torch
    names = ["scene", "clumps_outliers", "holes"]
    clouds = [KR.shapes()[n] for n in names]
    dev = [torch.from_numpy(c.copy()).cuda() for c in clouds]
    got = ctx.outlier_filter_batch(dev, points=True, **RAD2)
    kept_host = [c[_np(g["indices"])] for c, g in zip(clouds, got)]
    assert all(len(k) > 50 for k in kept_host)
    on_device = ctx.cluster_extract_batch([g["points"] for g in got], tolerance=0.5, min_cluster_size=3)
    on_host = ctx.cluster_extract_batch(kept_host, tolerance=0.5, min_cluster_size=3)
    for a, b in zip(on_device, on_host):
        assert a["n_clusters"] == b["n_clusters"] and a["n_clusters"] > 0
        for key in ("labels", "indices", "offsets"):
            assert _np(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


# ------------------------------------------------------------------ 6. capacity and side effects
def _raw_batch(wm, ctx, clouds, params, cap, out_stride=12):
    """the C entry with a capacity of its own (host memory) -> rc, offsets, indices, points, status"""
    p = wm.outlier_params(params)
    tab = (wm.OutlierScan * len(clouds))()
    for k, c in enumerate(clouds):
        tab[k].pts, tab[k].n = c.ctypes.data, len(c)
    total = sum(len(c) for c in clouds)
    idx = np.full(total, -7, np.int32)
    pts = np.full((total, out_stride // 4), -7.0, np.float32)
    offs = (C.c_size_t * (len(clouds) + 1))()
    status = (C.c_int * len(clouds))()
    rc = wm.lib().wm_outlier_filter_batch(ctx._h, tab, len(clouds), 12, wm.WM_MEM_HOST, C.byref(p), C.c_void_p(idx.ctypes.data),
                                          cap, C.c_void_p(pts.ctypes.data), out_stride, wm.WM_MEM_HOST, offs, None, None,
                                          None, status, None, None)
    return rc, [int(v) for v in offs], idx, pts, list(status)


@pytest.mark.parametrize("params", [STAT8, RAD2])
def test_cap_one_short_is_an_argument_error_with_the_true_offsets(wm, ctx, params):
    clouds = [np.ascontiguousarray(KR.shapes()[n]) for n in ("scene", "clumps_outliers")]
    full = ctx.outlier_filter_batch(clouds, points=True, **params)
    want_idx = np.concatenate([g["indices"] for g in full])
    want_pts = np.concatenate([g["points"] for g in full])
    kept = len(want_idx)
    want_offs = [0, len(full[0]["indices"]), kept]
    assert 1 < kept < sum(len(c) for c in clouds)
    rc, offs, idx, pts, status = _raw_batch(wm, ctx, clouds, params, kept)
    assert rc == wm.WM_OK and offs == want_offs and np.array_equal(idx[:kept], want_idx) and (idx[kept:] == -7).all()
    rc, offs, idx, pts, status = _raw_batch(wm, ctx, clouds, params, kept - 1)
    assert rc == wm.WM_ERR_ARG and offs == want_offs and status == [wm.WM_OK, wm.WM_OK]
    assert np.array_equal(idx[:kept - 1], want_idx[:kept - 1]) and (idx[kept - 1:] == -7).all()
    assert pts[:kept - 1].tobytes() == want_pts[:kept - 1].tobytes() and (pts[kept - 1:] == -7.0).all()


@pytest.mark.parametrize("params", [STAT8, RAD2])
def test_a_batch_of_one_is_the_single_call(wm, ctx, params):
    import torch
    cloud = KR.shapes()["holes"]
    for arr in (cloud, torch.from_numpy(cloud.copy()).cuda()):
        batch, singles = _against_singles(wm, ctx, [arr], "a batch of one", **params)
        got = ctx.outlier_filter_batch([arr], points=True, **params)[0]
        assert _np(got["points"]).tobytes() == cloud[_np(singles[0]["indices"])].tobytes()
    few = cloud[1:4]  # too few points for mean_k 8: the scan's status, the call is WM_OK
    got = ctx.outlier_filter_batch([few], **STAT8)[0]
    assert got["rc"] == wm.WM_NOT_CONVERGED and len(got["indices"]) == 0 and got["n_finite"] == 3
    rc, offs, idx, pts, status = _raw_batch(wm, ctx, [np.ascontiguousarray(cloud)], params, 10)
    one = ctx.outlier_filter(cloud, **params)
    assert rc == wm.WM_ERR_ARG and offs == [0, len(one["indices"])] and np.array_equal(idx[:10], one["indices"][:10])
    assert pts[:10].tobytes() == cloud[one["indices"][:10]].tobytes() and (idx[10:] == -7).all()


def test_registration_state_is_not_touched(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    scans = [KR.shapes()["clumps_outliers"], KR.shapes()["scene"]]
    runs = []
    for with_filters in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0)
            knn_a = c.debug_knn(1, 10)
            corr_a = c.correspondences()
            if with_filters:
                assert len(c.outlier_filter_batch(scans, **STAT8)[0]["indices"]) == 3000
                assert all(g["rc"] == wm.WM_OK for g in c.outlier_filter_batch(scans, points=True, **RAD2))
                assert all(g["rc"] == wm.WM_OK for g in c.outlier_filter_batch(scans, counts=False, **RAD2))
            corr_b = c.correspondences()
            knn_b = c.debug_knn(1, 10)
            b = c.icp_align(max_corr=3.0)
            assert corr_a[0].tobytes() == corr_b[0].tobytes() and corr_a[1].tobytes() == corr_b[1].tobytes()
            assert knn_a[0].tobytes() == knn_b[0].tobytes() and knn_a[1].tobytes() == knn_b[1].tobytes()
            assert c.sizes() == (len(ref_cloud), len(tgt_cloud))
            runs.append((a, b))
        finally:
            c.close()
    (a1, b1), (a2, b2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]


# ------------------------------------------------------------------ 7. lattices
def test_a_utm_scan_beside_one_at_the_origin_and_the_cell_rule(wm, ctx):
    clouds = [KR.shapes()["utm"], KR.shapes()["scene"], KR.shapes()["utm_plane"]]
    base_r = ctx.outlier_filter_batch(clouds, **RAD2)
    base_s = ctx.outlier_filter_batch(clouds, **STAT8)
    try:
        for div in (0.5, 8.0, 2.0):
            ctx.set_option("outlier_cell_div", div)
            for r in OR.RADII:
                _against_singles(wm, ctx, clouds, "div %g radius %g" % (div, r), method=1, radius=r,
                                 min_neighbors=OR.MIN_NEIGHBORS)
            got_r, _ = _against_singles(wm, ctx, clouds, "div %g" % div, **RAD2)
            got_s, _ = _against_singles(wm, ctx, clouds, "div %g" % div, **STAT8)
            for a, b in zip(got_r + got_s, base_r + base_s):
                _same_scan(wm, a, b, "div %g against the default" % div)
    finally:
        ctx.set_option("outlier_cell_div", 2.0)
