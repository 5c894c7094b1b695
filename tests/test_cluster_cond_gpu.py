"""wm_cluster_extract_cond (libwave_amd/csrc/wm_cluster.hip) on the GPU against tests/cluster_cond_reference.py: the
table of small shapes whose component counts are known by hand (a corner of floor and wall, a fan of turning normals,
pairs at exactly the threshold, NaN and zero attributes), cluster_reference's fourteen stress shapes with the normals
and curvatures wm_estimate_normals gives them, and one scene above the 256k sort switch.

Everything is compared EXACTLY -- labels, indices, offsets, the counters: the partition is a function of the float32
distances, dots and differences alone, all formed the same way on both sides.  The attributes are fetched ONCE from the
device and given to both the checker and the call, so no float disagreement enters.
tests/test_cluster_cond_reference_cpu.py holds the checker's two forms to each other."""
import ctypes as C

import numpy as np
import pytest

import cluster_cond_reference as CC
import cluster_reference as CR
import knn_reference as KR

pytestmark = pytest.mark.gpu

STATS = ("n_finite", "n_components", "n_clusters", "n_clustered", "largest")
KEYS = ("labels", "indices", "offsets")
_ATTR = {}


def _kw(angle, diff):
    kw = {}
    if angle is not None:
        kw["max_normal_angle"] = angle
    if diff is not None:
        kw["max_scalar_diff"] = diff
    return kw


def _host(got):
    if isinstance(got["indices"], np.ndarray):
        return got
    return dict(got, indices=got["indices"].cpu().numpy(), labels=got["labels"].cpu().numpy(),
                offsets=got["offsets"].cpu().numpy().view(np.uint32))


def _same(wm, got, ref, what):
    got = _host(got)
    assert got["rc"] == wm.WM_OK, what
    print("%s: %d clusters of %d components (want %d of %d), largest %d; %.3f ms on the device"
          % (what, got["n_clusters"], got["n_components"], ref["n_clusters"], ref["n_components"], got["largest"],
             got["kernel_ms"]))
    assert got["n_clusters"] == ref["n_clusters"] and got["n_out"] == ref["n_out"], what
    for k in STATS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    assert got["offsets"].dtype == np.uint32 and np.array_equal(got["offsets"], ref["offsets"]), what
    assert got["indices"].dtype == np.int32 and np.array_equal(got["indices"], ref["indices"]), what
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"]), what


def _same_bytes(a, b, what):
    a, b = _host(a), _host(b)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert [a[k] for k in STATS] == [b[k] for k in STATS] and (a["n_clusters"], a["n_out"]) == (b["n_clusters"], b["n_out"]), what


def device_attr(wm, cloud, key=None):
    """wm_estimate_normals (k = 10) of `cloud`, fetched once to the host: (nx, ny, nz, curvature) per point."""
    if key is not None and key in _ATTR:
        return _ATTR[key]
    c = wm.Context(0)
    try:
        c.set_source(cloud)  # (wm_estimate_normals wants both clouds set)
        c.set_target(cloud)
        attr = c.estimate_normals(1, k=CC.NORMAL_K)
    finally:
        c.close()
    attr.setflags(write=False)
    if key is not None:
        _ATTR[key] = attr
    return attr


# ------------------------------------------------------------------ the table
def test_the_table(wm, ctx):
    for what, (cloud, attr), tol, angle, diff, n_comp, largest in CC.table():
        ref = CC.components_brute(cloud, attr, tol, angle, diff)
        got = ctx.cluster_extract_cond(cloud, attr, tolerance=tol, **_kw(angle, diff))
        _same(wm, got, ref, what)
        assert got["n_components"] == n_comp and got["largest"] == largest[0], what
    corner, cattr = CC.shapes()["corner"]
    plain = ctx.cluster_extract(corner, tolerance=0.15)
    assert plain["n_clusters"] == 1 and plain["largest"] == 2048  # the floor and the wall are one object without a test
    split = ctx.cluster_extract_cond(corner, cattr, tolerance=0.15, max_normal_angle=30 * CC.DEG)
    assert split["n_clusters"] == 2 and np.diff(split["offsets"]).tolist() == [1024, 1024]
    for c in range(2):  # one cluster is the floor, the other the wall
        members = split["indices"][split["offsets"][c]:split["offsets"][c + 1]]
        assert len(np.unique(cattr[members, 2])) == 1
    for kw in (dict(middle_s=np.nan), dict(middle_normal=(0.0, 0.0, 0.0))):
        cloud, attr = CC.triple(**kw)
        cond = dict(max_scalar_diff=5.0) if "middle_s" in kw else dict(max_normal_angle=30 * CC.DEG)
        assert ctx.cluster_extract_cond(cloud, attr, tolerance=0.2, **cond)["labels"].tolist() == [0, 1, 0]


# ------------------------------------------------------------------ the stress shapes with the device's own normals
@pytest.mark.parametrize("name", KR.NAMES + sorted(CR.OWN))
def test_equals_the_checker(wm, ctx, name):
    cloud = CR.shapes()[name]
    attr = device_attr(wm, cloud, name)
    assert attr.shape == (len(cloud), 4) and attr.dtype == np.float32
    for tol in [t for n, t in CR.CASES if n == name]:
        for angle, diff in CC.CONDITIONS:
            ref = CC.brute_case(name, tol, attr, angle, diff)
            got = ctx.cluster_extract_cond(cloud, attr, tolerance=tol, **_kw(angle, diff))
            _same(wm, got, ref, "%s tolerance %.9g angle %s diff %s" % (name, tol, angle, diff))
        # no test: wm_cluster_extract's bytes, with and without attributes
        plain = ctx.cluster_extract(cloud, tolerance=tol)
        _same_bytes(ctx.cluster_extract_cond(cloud, None, tolerance=tol), plain, (name, tol))
        _same_bytes(ctx.cluster_extract_cond(cloud, attr, wm.cluster_cond(max_normal_angle=0.1, flags=0), tolerance=tol), plain,
                    (name, tol))
    if name == "holes":
        holes = [0, 17, 1500, len(cloud) - 1]
        assert (got["labels"][holes] == wm.WM_CLUSTER_NONE).all() and got["n_finite"] == 2996


@pytest.mark.parametrize("name,tol", [("scene", 2.0), ("holes", 2.0), ("noisy_plane", 0.5)])
def test_normals_left_on_the_device_give_the_host_paths_bytes(wm, ctx, name, tol):
    import torch
    cloud = CR.shapes()[name]
    dev = torch.from_numpy(cloud.copy()).cuda()
    c = wm.Context(0)
    try:
        c.set_source(dev)
        c.set_target(dev)
        dattr = c.estimate_normals(1, k=CC.NORMAL_K, out=torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda"))
    finally:
        c.close()
    attr = dattr.cpu().numpy()
    for angle, diff in CC.CONDITIONS:
        on_dev = ctx.cluster_extract_cond(dev, dattr, tolerance=tol, **_kw(angle, diff))
        assert on_dev["indices"].is_cuda and on_dev["labels"].is_cuda and on_dev["offsets"].is_cuda
        on_host = ctx.cluster_extract_cond(cloud, attr, tolerance=tol, **_kw(angle, diff))
        _same_bytes(on_dev, on_host, (name, angle, diff))
        _same(wm, on_dev, CC.components_brute(cloud, attr, tol, angle, diff), "%s on the device" % name)


# ------------------------------------------------------------------ representatives do not leak
@pytest.mark.parametrize("name,tol,angle,diff", [("scene", 2.0, 45 * CC.DEG, None), ("dups", 0.5, 10 * CC.DEG, 0.01),
                                                 ("corner", 0.15, 30 * CC.DEG, None)])
def test_row_permutations_give_the_same_clusters(wm, ctx, name, tol, angle, diff):
    if name == "corner":
        cloud, attr = CC.shapes()["corner"]
    else:
        cloud = CR.shapes()[name]
        attr = device_attr(wm, cloud, name)
    rng = np.random.default_rng(78)
    sets = []
    for trial in range(3):
        perm = np.arange(len(cloud)) if trial == 0 else rng.permutation(len(cloud))
        c, a = np.ascontiguousarray(cloud[perm]), np.ascontiguousarray(attr[perm])
        got = ctx.cluster_extract_cond(c, a, tolerance=tol, **_kw(angle, diff))
        _same(wm, got, CC.components_brute(c, a, tol, angle, diff), "%s permutation %d" % (name, trial))
        _same_bytes(got, ctx.cluster_extract_cond(c, a, tolerance=tol, **_kw(angle, diff)), (name, trial))
        off = got["offsets"]
        sets.append(sorted(tuple(sorted(perm[got["indices"][off[j]:off[j + 1]]].tolist())) for j in range(got["n_clusters"])))
    assert sets[0] == sets[1] == sets[2]


# ------------------------------------------------------------------ the cell rule
@pytest.mark.parametrize("name", ["lattice", "rails", "utm", "clumps_outliers"])
def test_the_cell_rule_changes_no_output(wm, ctx, name):
    cloud = CR.shapes()[name]
    attr = device_attr(wm, cloud, name)
    angle, diff = CC.CONDITIONS[3]
    try:
        for div in (0.5, 2.0, 8.0):
            ctx.set_option("cluster_cell_div", div)
            for tol in [t for n, t in CR.CASES if n == name]:
                _same(wm, ctx.cluster_extract_cond(cloud, attr, tolerance=tol, **_kw(angle, diff)),
                      CC.brute_case(name, tol, attr, angle, diff), "%s div %g tolerance %.9g" % (name, div, tol))
    finally:
        ctx.set_option("cluster_cell_div", 2.0)


# ------------------------------------------------------------------ plumbing
def _random_case(n, seed):
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    v = rng.normal(size=(n, 3))
    attr = np.c_[v / np.linalg.norm(v, axis=1, keepdims=True), rng.uniform(0, 1, n)].astype(np.float32)
    return cloud, attr


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_tiny_clouds(wm, ctx, n):
    cloud, attr = _random_case(n, n)
    for tol in (0.3, 5.0):
        for angle, diff in ((60 * CC.DEG, None), (None, 0.3), (60 * CC.DEG, 0.3)):
            _same(wm, ctx.cluster_extract_cond(cloud, attr, tolerance=tol, **_kw(angle, diff)),
                  CC.components_brute(cloud, attr, tol, angle, diff), "n %d tolerance %g %s %s" % (n, tol, angle, diff))


def _abi(wm, ctx, cloud, stride, attr, attr_stride, tol, cond, cap=None, cap_clusters=None, min_cluster_size=1):
    """The C ABI on host memory with explicit strides and capacities -> rc, n_clusters, n_out, labels, indices, offsets."""
    n = len(cloud)
    cap = n if cap is None else cap
    cap_clusters = n if cap_clusters is None else cap_clusters
    p = wm.cluster_params(tolerance=tol, min_cluster_size=min_cluster_size)
    idx, off, lab = np.full(cap + 1, -7, np.int32), np.full(cap_clusters + 2, 9, np.uint32), np.empty(n, np.int32)
    m, k = C.c_size_t(0), C.c_size_t(0)
    rc = wm.lib().wm_cluster_extract_cond(ctx._h, C.c_void_p(cloud.ctypes.data), n, stride, wm.WM_MEM_HOST,
                                          C.c_void_p(attr.ctypes.data), attr_stride, wm.WM_MEM_HOST, C.byref(p), C.byref(cond),
                                          C.c_void_p(lab.ctypes.data), C.c_void_p(idx.ctypes.data), cap,
                                          C.c_void_p(off.ctypes.data), cap_clusters, wm.WM_MEM_HOST, C.byref(k), C.byref(m), None)
    return rc, k.value, m.value, lab, idx, off


def test_attribute_strides_16_and_32(wm, ctx):
    cloud = CR.shapes()["scene"]
    attr = device_attr(wm, cloud, "scene")
    cond = wm.cluster_cond(max_normal_angle=45 * CC.DEG, max_scalar_diff=0.01)
    ref = CC.brute_case("scene", 2.0, attr, 45 * CC.DEG, 0.01)
    a32 = np.ascontiguousarray(np.c_[attr, np.full((len(attr), 4), np.nan, np.float32)], np.float32)  # (a payload behind)
    c32 = np.ascontiguousarray(np.c_[cloud, np.full((len(cloud), 5), 7.0, np.float32)], np.float32)
    for c, stride in ((cloud, 12), (c32, 32)):
        for a, astride in ((np.ascontiguousarray(attr), 16), (a32, 32)):
            rc, k, m, lab, idx, off = _abi(wm, ctx, c, stride, a, astride, 2.0, cond)
            assert rc == wm.WM_OK and (k, m) == (ref["n_clusters"], ref["n_out"])
            assert np.array_equal(lab, ref["labels"]) and np.array_equal(idx[:m], ref["indices"])
            assert np.array_equal(off[:k + 1], ref["offsets"])


def test_every_combination_of_memories_gives_the_same_bytes(wm, ctx):
    import torch
    cloud = CR.shapes()["holes"]
    attr = np.ascontiguousarray(device_attr(wm, cloud, "holes"))
    angle, diff = CC.CONDITIONS[3]
    first = ctx.cluster_extract_cond(cloud, attr, tolerance=2.0, **_kw(angle, diff))
    _same(wm, first, CC.brute_case("holes", 2.0, attr, angle, diff), "holes")
    for c in (cloud, torch.from_numpy(cloud.copy()).cuda()):
        for a in (attr, torch.from_numpy(attr.copy()).cuda()):
            for out_mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
                got = ctx.cluster_extract_cond(c, a, tolerance=2.0, out_mem=out_mem, **_kw(angle, diff))
                assert (out_mem == wm.WM_MEM_DEVICE) == (not isinstance(got["indices"], np.ndarray))
                _same_bytes(got, first, (type(c), type(a), out_mem))
    got = ctx.cluster_extract_cond(cloud, attr, tolerance=2.0, labels=False, **_kw(angle, diff))
    assert got["labels"] is None and got["indices"].tobytes() == first["indices"].tobytes()


def test_size_rule(wm, ctx):
    cloud, attr = CC.shapes()["fan"]
    got = ctx.cluster_extract_cond(cloud, attr, tolerance=0.2, max_normal_angle=4 * CC.DEG, min_cluster_size=2)
    assert got["rc"] == wm.WM_OK and got["n_clusters"] == 0 and got["n_components"] == 64 and got["offsets"].tolist() == [0]
    assert (got["labels"] == wm.WM_CLUSTER_REJECTED).all()  # min_cluster_size cuts the fan's singletons
    cloud = CR.shapes()["scene"]
    attr = device_attr(wm, cloud, "scene")
    full = CC.brute_case("scene", 2.0, attr, 45 * CC.DEG, None)
    assert (full["component_sizes"] == 1).any() and full["largest"] > 100
    for lo, hi in ((2, CR.INT_MAX), (20, CR.INT_MAX), (1, 100), (2, 100), (0, CR.INT_MAX), (30, 5)):
        ref = CR.with_size_rule(full, lo, hi)
        got = ctx.cluster_extract_cond(cloud, attr, tolerance=2.0, max_normal_angle=45 * CC.DEG, min_cluster_size=lo,
                                       max_cluster_size=hi)
        _same(wm, got, dict(ref, n_components=full["n_components"]), "scene sizes %d ... %d" % (lo, hi))
        assert np.array_equal(got["labels"] == wm.WM_CLUSTER_REJECTED, ref["labels"] == CR.REJECTED)


def test_capacities_one_short_are_argument_errors_with_the_true_counts(wm, ctx):
    cloud = CR.shapes()["scene"]
    attr = np.ascontiguousarray(device_attr(wm, cloud, "scene"))
    cond = wm.cluster_cond(max_normal_angle=45 * CC.DEG)
    ref = CR.with_size_rule(CC.brute_case("scene", 2.0, attr, 45 * CC.DEG, None), 2, CR.INT_MAX)
    kept, ncl = ref["n_out"], ref["n_clusters"]
    assert 1 < kept < len(cloud) and ncl > 1
    rc, k, m, _, idx, off = _abi(wm, ctx, cloud, 12, attr, 16, 2.0, cond, kept, ncl, 2)
    assert rc == wm.WM_OK and (k, m) == (ncl, kept)
    assert np.array_equal(idx, np.r_[ref["indices"], np.int32(-7)]) and np.array_equal(off, np.r_[ref["offsets"], np.uint32(9)])
    rc, k, m, _, idx, off = _abi(wm, ctx, cloud, 12, attr, 16, 2.0, cond, kept - 1, ncl, 2)
    assert rc == wm.WM_ERR_ARG and (k, m) == (ncl, kept)
    assert np.array_equal(idx, np.r_[ref["indices"][:kept - 1], np.int32(-7)])
    assert np.array_equal(off, np.r_[np.minimum(ref["offsets"], kept - 1), np.uint32(9)])
    rc, k, m, _, idx, off = _abi(wm, ctx, cloud, 12, attr, 16, 2.0, cond, kept, ncl - 1, 2)
    assert rc == wm.WM_ERR_ARG and (k, m) == (ncl, kept)
    assert np.array_equal(idx[:kept], ref["indices"]) and np.array_equal(off, np.r_[ref["offsets"][:ncl], np.uint32(9)])


def test_non_finite_points(wm, ctx):
    import torch
    nans = np.full((100, 3), np.nan, np.float32)
    nans[::3, 1] = np.inf
    nans[1::3, 0] = 1.0
    attr = np.tile(np.float32([0, 0, 1, 0.5]), (100, 1))
    for c, a in ((nans, attr), (torch.from_numpy(nans.copy()).cuda(), torch.from_numpy(attr.copy()).cuda())):
        got = _host(ctx.cluster_extract_cond(c, a, tolerance=0.5, max_normal_angle=0.5, max_scalar_diff=1.0))
        assert got["rc"] == wm.WM_OK and got["n_clusters"] == 0 and got["n_out"] == 0 and got["n_finite"] == 0
        assert len(got["labels"]) == 100 and (got["labels"] == wm.WM_CLUSTER_NONE).all() and got["offsets"].tolist() == [0]
    # a non-finite point with finite attributes is NONE; its neighbours go on without it
    cloud, cattr = CC.shapes()["corner"]
    cloud = cloud.copy()
    gone = [0, 5, 1000, 2047]
    cloud[gone, 0] = np.nan
    cloud[5, :] = np.inf
    ref = CC.components_brute(cloud, cattr, 0.15, 30 * CC.DEG, None)
    got = ctx.cluster_extract_cond(cloud, cattr, tolerance=0.15, max_normal_angle=30 * CC.DEG)
    _same(wm, got, ref, "corner with holes")
    assert (got["labels"][gone] == wm.WM_CLUSTER_NONE).all() and got["n_finite"] == 2044
    # a finite point with NaN attributes is a cluster of one
    cloud, cattr = CC.shapes()["corner"]
    cattr = cattr.copy()
    cattr[7] = np.nan
    got = ctx.cluster_extract_cond(cloud, cattr, tolerance=0.15, max_normal_angle=30 * CC.DEG, max_scalar_diff=1.0)
    _same(wm, got, CC.components_brute(cloud, cattr, 0.15, 30 * CC.DEG, 1.0), "corner with a NaN record")
    assert got["labels"][7] == 2 and got["n_clusters"] == 3 and got["offsets"].tolist() == [0, 1024, 2047, 2048]


# ------------------------------------------------------------------ one size above the 256k sort switch
def test_large_scene_against_the_kdtree(wm, ctx):
    cloud = CR.big_cloud()
    assert len(cloud) > 256 << 10
    attr = device_attr(wm, cloud)
    ref = CC.big_case(attr)
    assert ref["n_near"] > ref["n_edges"] > 0  # (the normal test refuses some of the near pairs)
    _same(wm, ctx.cluster_extract_cond(cloud, attr, tolerance=CC.BIG_TOLERANCE, max_normal_angle=CC.BIG_ANGLE), ref,
          "scene(%d) tolerance %g normal 30 deg" % (len(cloud), CC.BIG_TOLERANCE))


# ------------------------------------------------------------------ the context's other state
def test_state_is_not_touched(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    third = CR.shapes()["clumps_outliers"]
    attr = device_attr(wm, third, "clumps_outliers")
    tattr = device_attr(wm, tgt_cloud)
    runs = []
    for with_cluster in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)  # (the target's normals are cached on the context)
            nrm_a = c.estimate_normals(1, k=20)
            corr_a = c.correspondences()
            o1 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            plain_a = c.cluster_extract(third, tolerance=0.5)
            if with_cluster:
                got = c.cluster_extract_cond(third, attr, tolerance=0.5, max_normal_angle=10 * CC.DEG)
                assert got["rc"] == wm.WM_OK and got["n_components"] >= 14
                assert c.cluster_extract_cond(tgt_cloud, tattr, tolerance=0.3, max_scalar_diff=0.01)["rc"] == wm.WM_OK
            plain_b = c.cluster_extract(third, tolerance=0.5)  # after a conditional call: its old bytes
            _same_bytes(plain_a, plain_b, "wm_cluster_extract around a conditional call")
            assert plain_b["n_clusters"] == 14
            corr_b = c.correspondences()
            nrm_b = c.estimate_normals(1, k=20)
            o2 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            b = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            assert nrm_a.tobytes() == nrm_b.tobytes()
            assert corr_a[0].tobytes() == corr_b[0].tobytes() and corr_a[1].tobytes() == corr_b[1].tobytes()
            assert c.sizes() == (len(ref_cloud), len(tgt_cloud))
            for k in ("indices", "labels", "counts"):
                assert o1[k].tobytes() == o2[k].tobytes()
            runs.append((a, b, o2, nrm_b, corr_b))
        finally:
            c.close()
    (a1, b1, o1, n1, c1), (a2, b2, o2, n2, c2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]
    assert o1["indices"].tobytes() == o2["indices"].tobytes() and o1["counts"].tobytes() == o2["counts"].tobytes()
    assert n1.tobytes() == n2.tobytes() and c1[0].tobytes() == c2[0].tobytes() and c1[1].tobytes() == c2[1].tobytes()
