"""wm_cluster_extract (libwave_amd/csrc/wm_cluster.hip) on the GPU against tests/cluster_reference.py, on the stress
shapes of knn_reference.py and the checker's own two: collapsed grid axes, duplicates, far outliers, exact float ties
(the lattice and the rails: whole layers of pairs at exactly the tolerance), a 4096-point path with shuffled indices,
500 points on one spot, large offsets, non-finite points.

Everything is compared EXACTLY: the partition is a function of the float32 distances alone and the order of the
outputs is fixed by the contract (size, then smallest member index; indices ascending), so there is nothing to round.
tests/test_cluster_reference_cpu.py holds the checker's two forms to each other on every case used here."""
import ctypes as C

import numpy as np
import pytest

import cluster_reference as CR
import knn_reference as KR

pytestmark = pytest.mark.gpu

STATS = ("n_finite", "n_components", "n_clusters", "n_clustered", "largest")


def _same(wm, got, ref, what):
    assert got["rc"] == wm.WM_OK, what
    print("%s: %d clusters of %d components (want %d of %d), largest %d, %d points in clusters; %.3f ms on the device"
          % (what, got["n_clusters"], got["n_components"], ref["n_clusters"], ref["n_components"], got["largest"],
             got["n_clustered"], got["kernel_ms"]))
    assert got["n_clusters"] == ref["n_clusters"] and got["n_out"] == ref["n_out"], what
    for k in STATS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    assert got["offsets"].dtype == np.uint32 and np.array_equal(got["offsets"], ref["offsets"]), what
    assert got["indices"].dtype == np.int32 and np.array_equal(got["indices"], ref["indices"]), what
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"]), what


# ------------------------------------------------------------------ against the checker
@pytest.mark.parametrize("name", KR.NAMES + sorted(CR.OWN))
def test_equals_the_checker(wm, ctx, name):
    cloud = CR.shapes()[name]
    for tol in [t for n, t in CR.CASES if n == name]:
        ref = CR.brute_case(name, tol)
        got = ctx.cluster_extract(cloud, tolerance=tol)
        _same(wm, got, ref, "%s tolerance %.9g" % (name, tol))
        if name == "holes":
            holes = [0, 17, 1500, len(cloud) - 1]
            assert got["n_finite"] == 2996 and (got["labels"][holes] == wm.WM_CLUSTER_NONE).all()
            assert not np.isin(holes, got["indices"]).any()
        if name == "lattice" and tol == 0.5:  # every neighbour at exactly d2 == r2: strict, so nobody is joined
            assert got["n_clusters"] == 3375 and np.array_equal(got["indices"], np.arange(3375))
        if name == "helix" and tol == 0.1:
            assert got["n_clusters"] == 1 and got["largest"] == 4096


# ------------------------------------------------------------------ the size rule
@pytest.mark.parametrize("name,tol", [("scene", 2.0), ("shell", 0.5)])
def test_size_rule(wm, ctx, name, tol):
    cloud = CR.shapes()[name]
    full = CR.brute_case(name, tol)
    for lo, hi in ((2, CR.INT_MAX), (20, CR.INT_MAX), (1, 100), (2, 100), (20, 100), (0, CR.INT_MAX)):
        ref = CR.with_size_rule(full, lo, hi)
        got = ctx.cluster_extract(cloud, tolerance=tol, min_cluster_size=lo, max_cluster_size=hi)
        _same(wm, got, ref, "%s tolerance %g sizes %d ... %d" % (name, tol, lo, hi))
        assert np.array_equal(got["labels"] == wm.WM_CLUSTER_REJECTED, ref["labels"] == CR.REJECTED)
        assert got["n_components"] == full["n_components"]
        assert (ref["labels"] == CR.REJECTED).any() == (lo > 1 or hi < full["largest"])  # (both shapes have singletons)
    got = ctx.cluster_extract(cloud, tolerance=tol, min_cluster_size=30, max_cluster_size=5)  # max < min: legal
    assert got["rc"] == wm.WM_OK and got["n_clusters"] == 0 and got["n_out"] == 0 and got["offsets"].tolist() == [0]
    assert got["largest"] == 0 and got["n_components"] == full["n_components"]
    assert (got["labels"] == wm.WM_CLUSTER_REJECTED).all()


# ------------------------------------------------------------------ representatives do not leak
@pytest.mark.parametrize("name,tol", [("scene", 2.0), ("dups", 0.5), ("rails", 0.25)])
def test_row_permutations_give_the_same_clusters(wm, ctx, name, tol):
    cloud = CR.shapes()[name]
    rng = np.random.default_rng(77)
    sets = []
    for trial in range(3):
        perm = np.arange(len(cloud)) if trial == 0 else rng.permutation(len(cloud))
        c = np.ascontiguousarray(cloud[perm])
        got = ctx.cluster_extract(c, tolerance=tol)
        _same(wm, got, CR.components_brute(c, tol), "%s permutation %d" % (name, trial))
        again = ctx.cluster_extract(c, tolerance=tol)
        for k in ("labels", "indices", "offsets"):
            assert got[k].tobytes() == again[k].tobytes(), (name, trial, k)
        off = got["offsets"]
        sets.append(sorted(tuple(sorted(perm[got["indices"][off[j]:off[j + 1]]].tolist())) for j in range(got["n_clusters"])))
    assert sets[0] == sets[1] == sets[2]


# ------------------------------------------------------------------ the cell rule
@pytest.mark.parametrize("name", ["lattice", "rails", "utm", "clumps_outliers"])
def test_the_cell_rule_changes_no_output(wm, ctx, name):
    """option cluster_cell_div: cells of 2 tolerances (a box of 3 cells per axis), the default half, an eighth (17)"""
    cloud = CR.shapes()[name]
    try:
        for div in (0.5, 2.0, 8.0):
            ctx.set_option("cluster_cell_div", div)
            for tol in [t for n, t in CR.CASES if n == name]:
                _same(wm, ctx.cluster_extract(cloud, tolerance=tol), CR.brute_case(name, tol), "%s div %g tolerance %.9g" % (name, div, tol))
    finally:
        ctx.set_option("cluster_cell_div", 2.0)
    with pytest.raises(wm.WmError):
        ctx.set_option("cluster_cell_div", 0.25)


# ------------------------------------------------------------------ plumbing
def test_host_and_device_memory_and_strides_give_the_same_bytes(wm, ctx):
    import torch
    cloud = CR.shapes()["holes"]
    ref = CR.brute_case("holes", 2.0)
    first = ctx.cluster_extract(cloud, tolerance=2.0)
    _same(wm, first, ref, "holes")
    c4 = np.c_[cloud, np.full(len(cloud), 7.0, np.float32)].astype(np.float32)
    c8 = np.c_[c4, c4].astype(np.float32)
    for host in (cloud, c4):
        for arr in (host, torch.from_numpy(host.copy()).cuda()):
            for out_mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
                got = ctx.cluster_extract(arr, tolerance=2.0, out_mem=out_mem)
                if out_mem == wm.WM_MEM_DEVICE:
                    assert got["indices"].is_cuda and got["labels"].is_cuda and got["offsets"].is_cuda
                    got = dict(got, indices=got["indices"].cpu().numpy(), labels=got["labels"].cpu().numpy(),
                               offsets=got["offsets"].cpu().numpy().view(np.uint32))
                for k in ("indices", "labels", "offsets"):
                    assert got[k].tobytes() == first[k].tobytes(), (k, host.shape, type(arr), out_mem)
                assert [got[k] for k in STATS] == [first[k] for k in STATS]
    # stride 32 through the C ABI
    n = len(cloud)
    p = wm.cluster_params(tolerance=2.0)
    idx, off, lab = np.empty(n, np.int32), np.empty(n + 1, np.uint32), np.empty(n, np.int32)
    m, k = C.c_size_t(0), C.c_size_t(0)
    rc = wm.lib().wm_cluster_extract(ctx._h, C.c_void_p(c8.ctypes.data), n, 32, wm.WM_MEM_HOST, C.byref(p),
                                     C.c_void_p(lab.ctypes.data), C.c_void_p(idx.ctypes.data), n, C.c_void_p(off.ctypes.data),
                                     n, wm.WM_MEM_HOST, C.byref(k), C.byref(m), None)
    assert rc == wm.WM_OK and (k.value, m.value) == (ref["n_clusters"], ref["n_out"])
    assert np.array_equal(lab, ref["labels"]) and np.array_equal(idx[:m.value], ref["indices"])
    assert np.array_equal(off[:k.value + 1], ref["offsets"])


def test_labels_out_may_be_null(wm, ctx):
    cloud = CR.shapes()["scene"]
    got = ctx.cluster_extract(cloud, tolerance=2.0, labels=False)
    ref = CR.brute_case("scene", 2.0)
    assert got["rc"] == wm.WM_OK and got["labels"] is None
    assert np.array_equal(got["indices"], ref["indices"]) and np.array_equal(got["offsets"], ref["offsets"])


@pytest.mark.parametrize("device", [False, True])
def test_capacities_one_short_are_argument_errors_with_the_true_counts(wm, ctx, device):
    import torch
    cloud = CR.shapes()["scene"]
    ref = CR.with_size_rule(CR.brute_case("scene", 2.0), 2, CR.INT_MAX)
    kept, ncl = ref["n_out"], ref["n_clusters"]
    assert 1 < kept < len(cloud) and ncl > 1
    p = wm.cluster_params(tolerance=2.0, min_cluster_size=2)
    mem = wm.WM_MEM_DEVICE if device else wm.WM_MEM_HOST
    src = torch.from_numpy(cloud.copy()).cuda() if device else cloud

    def run(cap, cap_clusters):
        if device:
            idx = torch.full((kept + 1,), -7, dtype=torch.int32, device="cuda")
            off = torch.full((ncl + 2,), 9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ptrs = (src.data_ptr(), idx.data_ptr(), off.data_ptr())
        else:
            idx, off = np.full(kept + 1, -7, np.int32), np.full(ncl + 2, 9, np.uint32)
            ptrs = (src.ctypes.data, idx.ctypes.data, off.ctypes.data)
        m, k = C.c_size_t(0), C.c_size_t(0)
        rc = wm.lib().wm_cluster_extract(ctx._h, C.c_void_p(ptrs[0]), len(cloud), 12, mem, C.byref(p), None, C.c_void_p(ptrs[1]),
                                         cap, C.c_void_p(ptrs[2]), cap_clusters, mem, C.byref(k), C.byref(m), None)
        if device:
            idx, off = idx.cpu().numpy(), off.cpu().numpy().view(np.uint32)
        return rc, k.value, m.value, idx, off

    rc, k, m, idx, off = run(kept, ncl)
    assert rc == wm.WM_OK and (k, m) == (ncl, kept)
    assert np.array_equal(idx, np.r_[ref["indices"], np.int32(-7)]) and np.array_equal(off, np.r_[ref["offsets"], np.uint32(9)])
    rc, k, m, idx, off = run(kept - 1, ncl)  # one index short: the prefix, the offsets clamped to cap
    assert rc == wm.WM_ERR_ARG and (k, m) == (ncl, kept)
    assert np.array_equal(idx, np.r_[ref["indices"][:kept - 1], np.int32([-7, -7])])
    assert np.array_equal(off, np.r_[np.minimum(ref["offsets"], kept - 1), np.uint32(9)])
    rc, k, m, idx, off = run(kept, ncl - 1)  # one cluster short: all the indices, cap_clusters + 1 offsets
    assert rc == wm.WM_ERR_ARG and (k, m) == (ncl, kept)
    assert np.array_equal(idx[:kept], ref["indices"])
    assert np.array_equal(off, np.r_[ref["offsets"][:ncl], np.uint32([9, 9])])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_tiny_clouds(wm, ctx, n):
    rng = np.random.default_rng(n)
    cloud = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    for tol in (0.3, 5.0):
        _same(wm, ctx.cluster_extract(cloud, tolerance=tol), CR.components_brute(cloud, tol), "n %d tolerance %g" % (n, tol))


def test_empty_and_all_nan_clouds_are_ok_with_no_clusters(wm, ctx):
    got = ctx.cluster_extract(np.zeros((0, 3), np.float32), tolerance=0.5)
    assert got["rc"] == wm.WM_OK and got["n_clusters"] == 0 and got["n_out"] == 0 and got["offsets"].tolist() == [0]
    assert len(got["labels"]) == 0 and got["n_finite"] == 0
    nans = np.full((100, 3), np.nan, np.float32)
    nans[::3, 1] = np.inf
    nans[1::3, 0] = 1.0  # (x finite, y not)
    import torch
    for arr in (nans, torch.from_numpy(nans.copy()).cuda()):
        got = ctx.cluster_extract(arr, tolerance=0.5)
        lab = got["labels"] if isinstance(arr, np.ndarray) else got["labels"].cpu().numpy()
        off = got["offsets"] if isinstance(arr, np.ndarray) else got["offsets"].cpu().numpy()
        assert got["rc"] == wm.WM_OK and got["n_clusters"] == 0 and got["n_out"] == 0 and got["n_finite"] == 0
        assert len(lab) == 100 and (lab == wm.WM_CLUSTER_NONE).all() and off.tolist() == [0]


def test_a_tolerance_that_rounds_to_zero_and_one_that_covers_everything(wm, ctx):
    cloud = CR.shapes()["dups"]
    got = ctx.cluster_extract(cloud, tolerance=1e-30)  # r2 = 0 in float: d2 < 0 never holds, not even for duplicates
    assert got["n_clusters"] == len(cloud) and np.array_equal(got["indices"], np.arange(len(cloud)))
    got = ctx.cluster_extract(cloud, tolerance=1e-6)  # only the duplicates
    _same(wm, got, CR.components_brute(cloud, 1e-6), "dups 1e-6")
    assert got["n_clusters"] == 1000 and got["largest"] == 3
    got = ctx.cluster_extract(cloud, tolerance=1e6)
    assert got["n_clusters"] == 1 and np.array_equal(got["indices"], np.arange(len(cloud)))


# ------------------------------------------------------------------ one size above the 256k sort switch
@pytest.mark.parametrize("tol", CR.BIG_TOLERANCES)
def test_large_scene_against_the_kdtree(wm, ctx, tol):
    """0.1: 162 250 clusters (the ranking sort at size); 0.3: one component of 264 439 (the union-find at size)"""
    cloud, ref = CR.big_cloud(), CR.big_case(tol)
    assert len(cloud) > 256 << 10
    _same(wm, ctx.cluster_extract(cloud, tolerance=tol), ref, "scene(%d) tolerance %g" % (len(cloud), tol))


# ------------------------------------------------------------------ the context's other state
def test_state_is_not_touched(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    third = CR.shapes()["clumps_outliers"]
    runs = []
    for with_cluster in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)  # (the target's normals are cached on the context)
            o1 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            knn_a = c.debug_knn(1, 10)
            if with_cluster:
                got = c.cluster_extract(third, tolerance=0.5)
                assert got["rc"] == wm.WM_OK and got["n_clusters"] == 14
                assert c.cluster_extract(tgt_cloud, tolerance=0.3)["rc"] == wm.WM_OK
            knn_b = c.debug_knn(1, 10)
            o2 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            b = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            assert knn_a[0].tobytes() == knn_b[0].tobytes() and knn_a[1].tobytes() == knn_b[1].tobytes()
            assert c.sizes() == (len(ref_cloud), len(tgt_cloud))
            for k in ("indices", "labels", "counts"):
                assert o1[k].tobytes() == o2[k].tobytes()
            runs.append((a, b, o2))
        finally:
            c.close()
    (a1, b1, o1), (a2, b2, o2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]
    assert o1["indices"].tobytes() == o2["indices"].tobytes() and o1["counts"].tobytes() == o2["counts"].tobytes()


# ------------------------------------------------------------------ the pipeline
def test_ground_segmentation_into_clusters_on_the_device(wm, ctx, testscan):
    import torch
    scan = torch.from_numpy(np.ascontiguousarray(testscan[:, :3], np.float32)).cuda()
    _, kept, offsets = ctx.ground_segment_batch([scan], points=True)
    assert kept.is_cuda and len(kept) == offsets[-1] > 1000
    got = ctx.cluster_extract(kept, tolerance=0.5, min_cluster_size=10)
    assert got["indices"].is_cuda
    host = kept.cpu().numpy()
    ref = CR.components(host[:, :3], 0.5, min_cluster_size=10)
    got = dict(got, indices=got["indices"].cpu().numpy(), labels=got["labels"].cpu().numpy(),
               offsets=got["offsets"].cpu().numpy().view(np.uint32))
    _same(wm, got, ref, "obstacle points of the scan")
    assert got["n_clusters"] > 1 and (got["labels"] == wm.WM_CLUSTER_REJECTED).any()
