"""knn_search<K> (libwave_amd/csrc/wm_gicp_dev.hpp) on stress shapes, every list size (GPU, through the C ABI): the
neighbour lists themselves (wm_debug_knn) against tests/knn_reference.py's brute force -- every index equal, every
squared distance bit-identical -- and the products that stand on the search: k_gicp_cov against the oracle's matrices,
k_normals against plane_reference, the batched GICP's in-kernel grid against the one-pair path.

The shapes hit what the search does beyond a first box that already holds the answer: collapsed grid axes (planes,
a line, one point), long runs and far outliers (the box grows many times; the shell passes' x-extensions and `reach`),
exact float ties straddling the k-th place (a lattice, duplicates: the lower index must win wherever it sits), boxes
clamped at the grid's edge, large offsets, non-finite points (the caller-order query route), clouds of k - 1, k and
k + 1 points.  The first radius (option "knn_r0") and the target's cell size are swept to force many shell passes and
a single pass on the same data: no knob changes a result.

In every test the source and the target are the same cloud: the source goes through its own grid (source_grid) and its
Morton-ordered queries, the target through the level-0 search grid and that grid's order."""
import ctypes

import numpy as np
import pytest

import knn_reference as KR
import plane_reference as PR
from helpers import pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu

KS = [1, 3, 8, 10, 11, 16, 20, 23, 32]  # every instantiated list size (8, 10, 12, 16, 20, 24, 32), its top and below it


def _diff(gi, gd, wi, wd):
    """None when the lists are the expected ones (indices equal, distances bit-identical), else the first wrong place"""
    bad = (gi != wi) | (gd.view(np.uint32) != wd.view(np.uint32))
    if not bad.any():
        return None
    q = int(np.argmax(bad.any(1)))
    s = int(np.argmax(bad[q]))
    return "%d wrong rows; first: query %d slot %d got (%d, %r) want (%d, %r); row got %s want %s" % (
        bad.any(1).sum(), q, s, gi[q, s], float(gd[q, s]), wi[q, s], float(wd[q, s]), gi[q].tolist(), wi[q].tolist())


def _both(ctx, cloud):
    ctx.set_source(cloud)
    ctx.set_target(cloud)


def _check_lists(ctx, cloud, k, what, failures):
    wi, wd = KR.brute(cloud, k)
    for which in (0, 1):
        gi, gd = ctx.debug_knn(which, k)
        msg = _diff(gi, gd, wi, wd)
        if msg:
            failures.append("%s k = %d %s: %s" % (what, k, ("source", "target")[which], msg))


# ------------------------------------------------------------------ a. the lists
@pytest.mark.parametrize("name", KR.NAMES)
def test_lists_equal_brute_force(wm, ctx, name):
    """(plain equality holds on coincident points too: among equal distances the lower index comes first -- the
    (d2, index) rule -- so nothing weaker is asked of `point` and `dups`)"""
    cloud = KR.shapes()[name]
    _both(ctx, cloud)
    failures = []
    for k in KS:
        _check_lists(ctx, cloud, k, name, failures)
    print("\n".join(failures))
    assert not failures, failures[0]


def test_debug_knn_arguments_and_what_it_leaves_alone(wm, ctx):
    L = wm.lib()
    cloud = KR.shapes()["scene"]
    idx = np.zeros((len(cloud), 32), np.int32)
    d2 = np.zeros((len(cloud), 32), np.float32)
    ip, fp = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), d2.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.wm_debug_knn(ctx._h, 1, 10, ip, fp) == wm.WM_ERR_STATE  # no clouds yet
    ctx.set_source(cloud)
    assert L.wm_debug_knn(ctx._h, 0, 10, ip, fp) == wm.WM_ERR_STATE  # no target yet
    ctx.set_target(cloud)
    for which, k in ((2, 10), (-1, 10), (0, 0), (1, 33), (1, -1)):
        assert L.wm_debug_knn(ctx._h, which, k, ip, fp) == wm.WM_ERR_ARG
    assert L.wm_debug_knn(None, 0, 10, ip, fp) == wm.WM_ERR_ARG
    assert L.wm_debug_knn(ctx._h, 0, 10, None, fp) == wm.WM_ERR_ARG
    # cached covariances and normals survive it: the same bytes before and after, lists asked at other k in between
    cs, ct = ctx.gicp_covariances(10, 1e-3)
    nt = ctx.estimate_normals(1, 12)
    for which in (0, 1):
        ctx.debug_knn(which, 7)
        ctx.debug_knn(which, 24)
    cs2, ct2 = ctx.gicp_covariances(10, 1e-3)
    assert cs.tobytes() == cs2.tobytes() and ct.tobytes() == ct2.tobytes()
    assert nt.tobytes() == ctx.estimate_normals(1, 12).tobytes()


# ------------------------------------------------------------------ b. sizes
@pytest.mark.parametrize("k", [3, 10, 32])
def test_cloud_sizes_around_k_and_the_wave(wm, ctx, k):
    failures = []
    for n in sorted({k, k + 1, 63, 64, 65, 257, 1001}):
        if n < k:
            continue
        cloud = np.random.default_rng(1000 * k + n).uniform(-2, 2, (n, 3)).astype(np.float32)
        _both(ctx, cloud)
        _check_lists(ctx, cloud, k, "n = %d" % n, failures)
        if n == k:  # every list is the whole cloud (the box covers the grid: covers_all)
            for which in (0, 1):
                gi, _ = ctx.debug_knn(which, k)
                assert (np.sort(gi, axis=1) == np.arange(n)).all()
    print("\n".join(failures))
    assert not failures, failures[0]


@pytest.mark.parametrize("k", [3, 10, 32])
def test_one_point_too_few_is_not_converged(wm, ctx, k):
    L = wm.lib()
    n = k - 1
    cloud = np.random.default_rng(k).uniform(-2, 2, (n, 3)).astype(np.float32)
    _both(ctx, cloud)
    idx = np.zeros((n, k), np.int32)
    d2 = np.zeros((n, k), np.float32)
    nrm = np.zeros((n, 4), np.float32)
    cov = np.zeros((n, 9), np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    for which in (0, 1):
        assert L.wm_debug_knn(ctx._h, which, k, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                              d2.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == wm.WM_NOT_CONVERGED
        assert L.wm_estimate_normals(ctx._h, which, k, ctypes.c_void_p(nrm.ctypes.data), wm.WM_MEM_HOST) == wm.WM_NOT_CONVERGED
    assert L.wm_gicp_covariances(ctx._h, k, 1e-3, cov.ctypes.data_as(dp), cov.ctypes.data_as(dp)) == wm.WM_NOT_CONVERGED
    # a non-finite point does not count: k points of which one is NaN are one too few as well
    holed = np.r_[cloud, np.float32([[np.nan, 0, 0]])]
    _both(ctx, holed)
    idx = np.zeros((k, k), np.int32)
    d2 = np.zeros((k, k), np.float32)
    for which in (0, 1):
        assert L.wm_debug_knn(ctx._h, which, k, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                              d2.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == wm.WM_NOT_CONVERGED


# ------------------------------------------------------------------ c. no knob changes a result
@pytest.mark.parametrize("name", ["noisy_plane", "lattice", "shell", "scene", "dups"])
def test_first_radius_and_cell_size_change_nothing(wm, ctx, name):
    """knn_r0 = 0.25 cells: several shell passes per query; 8: one pass; the target's cells of 0.15 m (far below the point
    spacing: many empty cells, many passes) and 4 m (hundreds of points per cell).  (None of these shapes has far outliers
    or a large offset, where a 0.15 m lattice would be enormous.)"""
    cloud = KR.shapes()[name]
    failures = []
    try:
        for k in (10, 20):
            first = None
            for r0 in (0.25, 0.0, 8.0):
                for cell in (0.0, 0.15, 4.0):
                    ctx.set_option("knn_r0", r0)
                    ctx.set_grid_cell(cell)
                    _both(ctx, cloud)  # (covariances are cached per (k, eps) until a cloud changes)
                    what = "%s knn_r0 = %g cell = %g" % (name, r0, cell)
                    _check_lists(ctx, cloud, k, what, failures)
                    cov = ctx.gicp_covariances(k, 1e-3)
                    if first is None:
                        first = cov
                    elif not (cov[0].tobytes() == first[0].tobytes() and cov[1].tobytes() == first[1].tobytes()):
                        failures.append("%s k = %d: covariances differ from the first setting's" % (what, k))
    finally:
        ctx.set_option("knn_r0", 0.0)
        ctx.set_grid_cell(0.0)
    print("\n".join(failures))
    assert not failures, failures[0]


# ------------------------------------------------------------------ d. the product kernels
@pytest.mark.parametrize("name", KR.NAMES)
def test_covariances_match_the_oracle_on_stress_shapes(wm, ctx, oracle, name):
    """test_gicp_gpu.py's contract (bit-identical matrices) where the box grows; `holes`: the finite points, addressed by
    caller index"""
    cloud = KR.shapes()[name]
    finite = np.isfinite(cloud).all(1)
    _both(ctx, cloud)
    failures = []
    for k in (3, 8, 10, 12, 16, 20, 24, 32):
        want = oracle.gicp_covariances(cloud[finite], k=k, eps=1e-3)
        for which, got in zip(("source", "target"), ctx.gicp_covariances(k, 1e-3)):
            got = got[finite]
            if not np.array_equal(got, want):
                bad = (got != want).any((1, 2))
                failures.append("%s k = %d %s: %d matrices differ (first: point %d), max |diff| %.3e" % (
                    name, k, which, bad.sum(), np.nonzero(finite)[0][np.argmax(bad)], np.abs(got - want).max()))
    print("\n".join(failures))
    assert not failures, failures[0]


@pytest.mark.parametrize("name", KR.NORMAL_SHAPES)
def test_normals_match_the_reference_at_every_list_size(wm, ctx, name):
    """k = 20 is tests/test_icp_plane_gpu.py's; here the other instantiations of k_normals, with that file's rules and
    bounds (1e-6 rad, 1e-6 curvature, unit length, n . p <= 0) and at most 1 % left out (the reference alone leaves out
    0.1 % at the most: tests/test_knn_reference_cpu.py).  k = 3 is absent on purpose: three points are always coplanar."""
    cloud = KR.shapes()[name]
    _both(ctx, cloud)
    worst = [0.0, 0.0]
    for k in KR.NORMAL_KS:
        ref = PR.normals(cloud, k, nbrs=KR.brute(cloud, k + 1), origin=KR.normal_origin(name))
        for which in (1, 0):
            got = ctx.estimate_normals(which, k)
            ang, curv = PR.check_normals(got, cloud, k, "%s k = %d (%s)" % (name, k, ("source", "target")[which]), ref=ref,
                                         cap=KR.NORMAL_CAP)
            worst = [max(worst[0], ang), max(worst[1], curv)]
    print("%s: over k = %s, max angle %.3e rad, max curvature diff %.3e" % (name, KR.NORMAL_KS, worst[0], worst[1]))


def test_normals_of_a_line_and_of_one_point(wm, ctx):
    """two eigenvalues tie (no angle to compare): unit length or zero and never NaN on the line, zero on coincident points"""
    S = KR.shapes()
    for k in KR.NORMAL_KS:
        _both(ctx, S["point"])
        for which in (1, 0):
            assert np.array_equal(ctx.estimate_normals(which, k), np.zeros((len(S["point"]), 4), np.float32))
        _both(ctx, S["line"])
        for which in (1, 0):
            got = ctx.estimate_normals(which, k)
            assert np.isfinite(got).all()
            length = np.linalg.norm(got[:, :3].astype(np.float64), axis=1)
            assert ((np.abs(length - 1.0) < 1e-6) | (length == 0)).all()
            assert (np.abs(got[:, 3]) <= 1e-6).all()  # (curvature: the smallest eigenvalue of a rank-1 covariance)


# ------------------------------------------------------------------ e. the batched path's own grid
def test_batched_gicp_builds_the_same_neighbourhoods(wm, ctx):
    """gs_covariances (wm_gicp_small.hip) runs knn_search on a grid built inside the kernel: per pair the status and the
    iteration count of the one-pair path, the pose within the header's 1e-6 m / 1e-6 rad"""
    S = KR.shapes()
    T = synth.make_T((0.2, 0.1, 0), (0, 0, 0.02))
    names = ["noisy_plane", "shell", "scene", "clumps_outliers"]
    pairs = [(S[n], synth.transform_points(S[n], T)) for n in names]
    got = ctx.gicp_batch_match(pairs)
    assert len(got) == len(pairs)
    for name, (ref, tgt), g in zip(names, pairs, got):
        ctx.set_source(ref)
        ctx.set_target(tgt)
        one = ctx.gicp_align()
        print("%s: rc %d / %d, iterations %d / %d" % (name, g["rc"], one["rc"], g["iterations"], one["iterations"]))
        assert g["rc"] == one["rc"], name
        assert g["iterations"] == one["iterations"], name
        if g["rc"] == wm.WM_OK:
            dt, ang = pose_error(g["T"], one["T"])
            print("%s: |dt| %.3e m, angle %.3e rad" % (name, dt, ang))
            assert dt <= 1e-6 and ang <= 1e-6, (name, dt, ang)
