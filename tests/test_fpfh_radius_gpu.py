"""wm_normals_radius and wm_fpfh_radius (libwave_amd/csrc/wm_fpfh_radius.hip) on the GPU against
tests/fpfh_radius_reference.py.

Normals: the nine integer sums and n_s EQUAL the checker's; normals_out equals wm_normal_from_sums on those sums bit for
bit (one text for host and device).  First walk: the device's counts equal the checker's on the device's own normals,
except at points with a pair whose f1 bin coordinate (float64) lies within 1e-4 of an integer -- atan2f is the one
function of the rule that is not bit-defined.  There the f2 and f3 blocks are still equal, the f1 block has the same sum
and is within L1 distance 2 per such pair; the share of such points may be what tests/test_fpfh_radius_reference_cpu.py
measured for the radius (RR.RISKY_SHARE: 1.6 % at 6 spacings, 1.8 % at 10) plus one percentage point.  Second walk: the
checker's weighting of the device's own counts equals fpfh_out bit for bit, at every point."""
import math

import numpy as np
import pytest

import fpfh_radius_reference as RR
import fpfh_reference as FR
import iss_reference as IR

pytestmark = pytest.mark.gpu

F = np.float32
CLOUDS = ["scene", "rings", "scan"]


@pytest.fixture(scope="module")
def dev(wm):
    c = wm.Context(0)
    yield c
    c.close()


def host(a):
    if a is None:
        return None
    if hasattr(a, "cpu"):
        import torch
        a = a.cpu()
        return a.view(torch.int16).numpy().view(np.uint16) if a.dtype == torch.uint16 else a.numpy()
    return np.asarray(a)


def check_normals(wm, got, cloud, radius, ref=None):
    """sums and counts EQUAL the checker's; the records equal the host finish on those sums bit for bit"""
    ref = ref if ref is not None else RR.normal_sums(cloud, radius)
    sums, counts, nrm = host(got["sums"]), host(got["counts"]), host(got["normals"])
    assert got["rc"] == 0
    assert np.array_equal(counts, ref["counts"])
    assert np.array_equal(sums, ref["sums"])
    assert got["n_finite"] == int(ref["finite"].sum())
    want = np.zeros((len(cloud), 4), F)
    for i in np.nonzero(ref["finite"])[0]:
        want[i] = wm.normal_from_sums(sums[i], counts[i], ref["x"], cloud[i])
    assert nrm.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    return nrm


def check_fpfh(got, cloud, nrm, radius, max_risky=1.0, what=""):
    """-> the share of f1-risky points"""
    assert got["rc"] == 0, what
    cloud = np.ascontiguousarray(np.asarray(cloud)[:, :3], F)
    spfh, n_f, out = host(got["spfh"]).astype(np.int32), host(got["counts"]), host(got["fpfh"])
    pairs = RR.feature_pairs(cloud, radius)
    want, want_n, risky = RR.spfh(cloud, nrm, radius, pairs_=pairs)
    assert np.array_equal(n_f, want_n), what
    sure = risky == 0
    assert np.array_equal(spfh[sure], want[sure]), what
    assert np.array_equal(spfh[:, 11:], want[:, 11:]), what
    g1, w1 = spfh[~sure, :11], want[~sure, :11]
    assert np.array_equal(g1.sum(axis=1), w1.sum(axis=1)), what
    assert np.all(np.abs(g1 - w1).sum(axis=1) <= 2 * risky[~sure]), what
    share = float((~sure).mean())
    print("%s: f1-risky points %.2f %%, max neighbours %d" % (what, 100 * share, got["max_neighbors"]))
    assert share <= max_risky, what
    # the second walk on the device's own counts: bit for bit
    ref = RR.weight(spfh, cloud, nrm, radius, pairs_=pairs)
    assert out.view(np.uint32).tobytes() == ref.view(np.uint32).tobytes(), what
    finite = np.isfinite(cloud).all(axis=1)
    assert got["n_finite"] == int(finite.sum()), what
    assert got["n_valid"] == int((finite & np.any(np.asarray(nrm)[:, :3] != 0, axis=1)).sum()), what
    assert got["max_neighbors"] == max(int(want_n.max()), 0), what
    return share


def run_both(wm, dev, cloud, rn, rf, max_risky=1.0, what=""):
    cloud = np.ascontiguousarray(cloud, F)
    nrm = check_normals(wm, dev.normals_radius(cloud, rn, counts=True, sums=True), cloud, rn)
    got = dev.fpfh_radius(cloud, rf, normal_radius=rn, counts=True)
    check_fpfh(got, cloud, nrm, rf, max_risky, what)
    return got, nrm


def key(g):
    return tuple(host(g[k]).tobytes() for k in ("fpfh", "spfh", "counts")) + (g["rc"], g["n_finite"], g["n_valid"], g["max_neighbors"])


# ------------------------------------------------------------------ the three clouds, both radii
@pytest.mark.parametrize("mult", RR.RADII)
@pytest.mark.parametrize("name", CLOUDS)
def test_normals_equal_the_checker(wm, dev, name, mult):
    cloud = np.array(FR.clouds()[name])
    rn, rf = RR.radii(name, mult)
    check_normals(wm, dev.normals_radius(cloud, rn, counts=True, sums=True), cloud, rn, RR.normal_reference(name, mult))
    check_normals(wm, dev.normals_radius(cloud, rf, counts=True, sums=True), cloud, rf)  # (the feature radius: more neighbours)


@pytest.mark.parametrize("mult", RR.RADII)
@pytest.mark.parametrize("name", CLOUDS)
def test_both_walks_on_the_clouds(wm, dev, name, mult):
    cloud = np.array(FR.clouds()[name])
    rn, rf = RR.radii(name, mult)
    nrm = host(dev.normals_radius(cloud, rn)["normals"])
    got = dev.fpfh_radius(cloud, rf, normal_radius=rn, counts=True)
    cap = min(RR.RISKY_SHARE[mult] + 0.01, 0.05)
    check_fpfh(got, cloud, nrm, rf, cap, "%s %d x" % (name, mult))
    assert got["n_valid"] > 0.6 * len(cloud)


# ------------------------------------------------------------------ shapes where the kernels can go wrong
@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 193])
def test_sizes_around_the_wave(wm, dev, n, spread):
    cloud = IR.dense_cloud(193)[:n] if spread else RR.dense_ball(n, 1.0)
    got, nrm = run_both(wm, dev, cloud, 0.6 if spread else 1.0, 1.0, what="n = %d" % n)
    if not spread:
        assert got["max_neighbors"] == n - 1  # one ball: everybody is everybody's neighbour
    if n < 3:
        assert not nrm.any() and not host(got["fpfh"]).any()


def test_no_neighbour_and_exactly_two(wm, dev):
    """a lonely point: n_s = 1, zeros; a triple: n_s = 3, a normal; a couple: n_s = 2, zeros"""
    cloud = np.array([[10, 0, 0], [0, 5, 1], [0.3, 5, 1], [0, 5.3, 1.1], [-7, -7, 2], [-7.2, -7, 2]], F)
    got = dev.normals_radius(cloud, 1.0, counts=True, sums=True)
    nrm = check_normals(wm, got, cloud, 1.0)
    assert list(host(got["counts"])) == [1, 3, 3, 3, 2, 2]
    assert not nrm[0].any() and not nrm[4:].any() and np.all(np.abs(np.linalg.norm(nrm[1:4, :3], axis=1) - 1) < 1e-6)
    f = dev.fpfh_radius(cloud, 1.0, normal_radius=1.0, counts=True)
    check_fpfh(f, cloud, nrm, 1.0, what="lonely")
    assert list(host(f["counts"])) == [0, 2, 2, 2, 1, 1] and f["n_valid"] == 3
    assert not host(f["fpfh"])[[0, 4, 5]].any()


def test_a_pair_at_exactly_r2_is_out_and_one_ulp_below_is_in(wm, dev):
    at = np.array([[0, 0, 0], [0.5, 0, 0]], F)
    below = np.array([[0, 0, 0], [np.nextafter(F(0.5), F(0)), 0, 0]], F)
    up = np.tile(F([0, 0, 1, 0]), (2, 1))
    assert list(host(dev.normals_radius(at, 0.5, counts=True)["counts"])) == [1, 1]
    assert list(host(dev.normals_radius(below, 0.5, counts=True)["counts"])) == [2, 2]
    assert list(host(dev.fpfh_radius(at, 0.5, normals=up, counts=True)["counts"])) == [0, 0]
    g = dev.fpfh_radius(below, 0.5, normals=up, counts=True)
    assert list(host(g["counts"])) == [1, 1]
    check_fpfh(g, below, up, 0.5, what="one ulp below")
    assert host(g["spfh"]).sum() == 6


def test_duplicates_and_the_clamp(wm, dev):
    sub = np.array(FR.clouds()["scan"][:600])
    s = IR.median_spacing(sub)
    rn, rf = 4.0 * s, 8.0 * s
    cloud = np.r_[sub, sub[:150], sub[:50] + F([rf / 300.0, 0, 0])].astype(F)  # exact duplicates; neighbours at r / 300
    got, nrm = run_both(wm, dev, cloud, rn, rf, what="duplicates")
    _, _, i, j, d2 = RR.feature_pairs(cloud, rf)
    assert (d2 < IR.r2_of(rf) * F(2.0 ** -16)).sum() >= 100  # the clamp is at work
    assert np.array_equal(host(got["fpfh"])[:150], host(got["fpfh"])[600:750])  # a duplicate has its twin's row


def test_non_finite_rows_and_an_all_nan_cloud(wm, dev):
    sub = np.array(FR.clouds()["scan"][:1500])
    s = IR.median_spacing(sub)
    bad = sub.copy()
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    got, nrm = run_both(wm, dev, bad, 4.0 * s, 8.0 * s, what="nan-inf")
    out = ~np.isfinite(bad).all(1)
    assert out.sum() > 300 and np.all(host(got["counts"])[out] == -1) and not host(got["fpfh"])[out].any()
    assert not nrm[out].any() and got["n_valid"] > 300
    nan = np.full((70, 3), np.nan, F)
    g = dev.normals_radius(nan, 1.0, counts=True, sums=True)
    assert g["rc"] == 0 and g["n_finite"] == 0 and not host(g["normals"]).any() and np.all(host(g["counts"]) == -1)
    assert not host(g["sums"]).any()
    g = dev.fpfh_radius(nan, 1.0, normal_radius=0.5, counts=True)
    assert g["rc"] == 0 and (g["n_finite"], g["n_valid"], g["max_neighbors"]) == (0, 0, 0)
    assert not host(g["fpfh"]).any() and not host(g["spfh"]).any() and np.all(host(g["counts"]) == -1)


def test_zero_normals_own_and_neighbours(wm, dev):
    cloud = np.array(FR.clouds()["scene"][:1200])
    s = IR.median_spacing(cloud)
    rn, rf = 4.0 * s, 8.0 * s
    nrm = host(dev.normals_radius(cloud, rn)["normals"]).copy()
    nrm[::3] = 0  # a third of the points without a normal: no row of their own, no part in their neighbours' counts
    got = dev.fpfh_radius(cloud, rf, normals=nrm, counts=True)
    check_fpfh(got, cloud, nrm, rf, what="zeroed normals")
    assert not host(got["fpfh"])[::3].any() and not host(got["spfh"])[::3].any()
    assert got["n_valid"] == int(np.any(nrm[:, :3] != 0, axis=1).sum())


def test_a_cloud_far_from_the_origin_and_a_radius_larger_than_the_cloud(wm, dev):
    sub = np.array(FR.clouds()["scene"][:900])
    far = (sub.astype(np.float64) + [1.0e4, -1.0e4, 1.0e4]).astype(F)
    s = IR.median_spacing(far)
    run_both(wm, dev, far, 4.0 * s, 8.0 * s, what="far")
    small = np.array(FR.clouds()["scan"][:300])
    got, _ = run_both(wm, dev, small, 500.0, 1000.0, what="whole cloud")
    assert got["max_neighbors"] == 299
    assert np.all(host(dev.normals_radius(small, 500.0, counts=True)["counts"]) == 300)


def test_the_neighbour_limit(wm, dev):
    """8 192 points in one ball: 8 191 neighbours each, WM_OK.  One more: WM_ERR_ARG with the true maximum."""
    ball = RR.dense_ball(8193, 1.0)
    assert len(np.unique(ball, axis=0)) == 8193
    nrm = np.tile(F([0, 0, 1, 0]), (8193, 1))
    ok = dev.fpfh_radius(ball[:8192], 1.0, normals=nrm[:8192], counts=True)
    assert ok["rc"] == wm.WM_OK and ok["max_neighbors"] == 8191 and np.all(host(ok["counts"]) == 8191)
    spfh = host(ok["spfh"]).astype(np.int64)
    assert np.all(spfh.reshape(-1, 3, 11).sum(axis=2) <= 8191) and spfh.reshape(-1, 3, 11).sum(axis=2).max() > 8000
    sums = host(ok["fpfh"]).reshape(-1, 3, 11).astype(np.float64).sum(axis=2)
    assert np.all(np.abs(sums - 100) < 1e-3)
    over = dev.fpfh_radius(ball, 1.0, normals=nrm, counts=True)
    assert over["rc"] == wm.WM_ERR_ARG and over["max_neighbors"] == 8192
    # the call after a refused one is clean
    again = dev.fpfh_radius(ball[:8192], 1.0, normals=nrm[:8192], counts=True)
    assert key(again) == key(ok)


# ------------------------------------------------------------------ determinism
def test_two_calls_permutations_and_the_cell_size_change_no_byte(wm, dev):
    name = "rings"
    cloud = np.array(FR.clouds()[name])
    rn, rf = RR.radii(name, 6)
    base_n = dev.normals_radius(cloud, rn, counts=True, sums=True)
    base = dev.fpfh_radius(cloud, rf, normal_radius=rn, counts=True)
    nkey = lambda g: tuple(host(g[k]).tobytes() for k in ("normals", "counts", "sums"))  # noqa: E731
    assert nkey(dev.normals_radius(cloud, rn, counts=True, sums=True)) == nkey(base_n)
    assert key(dev.fpfh_radius(cloud, rf, normal_radius=rn, counts=True)) == key(base)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(cloud))
        moved = np.ascontiguousarray(cloud[perm])
        g = dev.normals_radius(moved, rn, counts=True, sums=True)
        for k in ("normals", "counts", "sums"):
            assert host(g[k]).tobytes() == host(base_n[k])[perm].tobytes(), k
        g = dev.fpfh_radius(moved, rf, normal_radius=rn, counts=True)
        for k in ("fpfh", "spfh", "counts"):
            assert host(g[k]).tobytes() == host(base[k])[perm].tobytes(), k
    try:
        for div in (0.5, 1.0, 2.0, 4.0, 8.0):
            dev.set_option("fpfh_cell_div", div)
            assert nkey(dev.normals_radius(cloud, rn, counts=True, sums=True)) == nkey(base_n), div
            assert key(dev.fpfh_radius(cloud, rf, normal_radius=rn, counts=True)) == key(base), div
        with pytest.raises(wm.WmError):
            dev.set_option("fpfh_cell_div", 0.25)
    finally:
        dev.set_option("fpfh_cell_div", 2.0)


# ------------------------------------------------------------------ the interface
def test_memory_spaces_strides_and_given_normals(wm, dev):
    import torch
    name = "scan"
    cloud = np.array(FR.clouds()[name])
    rn, rf = RR.radii(name, 6)
    base_n = dev.normals_radius(cloud, rn, counts=True, sums=True)
    base = dev.fpfh_radius(cloud, rf, normal_radius=rn, counts=True)
    nkey = lambda g: tuple(host(g[k]).tobytes() for k in ("normals", "counts", "sums"))  # noqa: E731

    def wide(a, w):
        out = np.full((len(a), w), 7.5, F)
        out[:, :3] = a
        return out

    assert key(dev.fpfh_radius(wide(cloud, 4), rf, normal_radius=rn, counts=True)) == key(base)
    for w in (3, 4, 8):  # strides 12, 16, 32 in device memory; 32 in host memory through a CPU tensor
        d = torch.from_numpy(wide(cloud, w)).cuda()
        g = dev.normals_radius(d, rn, counts=True, sums=True)
        assert g["normals"].is_cuda and g["counts"].is_cuda and g["sums"].is_cuda and nkey(g) == nkey(base_n)
        g = dev.fpfh_radius(d, rf, normal_radius=rn, counts=True)
        assert g["fpfh"].is_cuda and g["spfh"].is_cuda and g["counts"].is_cuda and key(g) == key(base)
        g = dev.fpfh_radius(d, rf, normal_radius=rn, counts=True, out_mem=wm.WM_MEM_HOST)
        assert isinstance(g["fpfh"], np.ndarray) and key(g) == key(base)
    g = dev.fpfh_radius(torch.from_numpy(wide(cloud, 8)), rf, normal_radius=rn, counts=True, out_mem=wm.WM_MEM_DEVICE)
    assert g["fpfh"].is_cuda and key(g) == key(base)
    assert nkey(dev.normals_radius(torch.from_numpy(wide(cloud, 8)), rn, counts=True, sums=True)) == nkey(base_n)
    # given normals give the bytes of estimated ones, in both memories; `out` is filled in place
    nrm = host(base_n["normals"])
    assert key(dev.fpfh_radius(cloud, rf, normals=nrm, counts=True)) == key(base)
    dcloud = torch.from_numpy(cloud).cuda()
    out = torch.full((len(cloud), 33), -1.0, dtype=torch.float32, device="cuda:0")
    g = dev.fpfh_radius(dcloud, rf, normals=torch.from_numpy(nrm).cuda(), counts=True, out=out)
    assert g["fpfh"] is out and key(g) == key(base)
    # no optional output at all
    g = dev.fpfh_radius(cloud, rf, normal_radius=rn)
    assert g["spfh"] is None and g["counts"] is None and g["fpfh"].tobytes() == host(base["fpfh"]).tobytes()
    g = dev.normals_radius(cloud, rn)
    assert g["counts"] is None and g["sums"] is None and g["normals"].tobytes() == host(base_n["normals"]).tobytes()
    assert base["kernel_ms"] > 0 and base["spfh_ms"] > 0 and base["weight_ms"] > 0 and base["normals_ms"] > 0


def test_argument_errors(wm, dev):
    cloud = np.array(FR.clouds()["scan"][:100])
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-20, 1e20):
        with pytest.raises(wm.WmError):
            dev.normals_radius(cloud, bad)
        with pytest.raises(wm.WmError):
            dev.fpfh_radius(cloud, bad, normal_radius=0.5)
        with pytest.raises(wm.WmError):
            dev.fpfh_radius(cloud, 1.0, normal_radius=bad)
    with pytest.raises(wm.WmError):
        dev.fpfh_radius(cloud, 1.0)  # neither normals nor a normal radius
    # a normal radius that is not read may be anything; the call after the refused ones is clean
    nrm = host(dev.normals_radius(cloud, 0.5)["normals"])
    a = dev.fpfh_radius(cloud, 1.0, normal_radius=float("nan"), normals=nrm, counts=True)
    b = dev.fpfh_radius(cloud, 1.0, normal_radius=0.5, counts=True)
    assert key(a) == key(b)


# ------------------------------------------------------------------ state
def test_the_registration_state_and_the_other_workspaces_are_untouched(wm):
    scan = np.ascontiguousarray(FR.clouds()["scan"])
    moved = (scan.astype(np.float64) + [0.3, 0.1, 0.0]).astype(F)
    rn, rf = RR.radii("scan", 6)
    c = wm.Context(0)
    try:
        c.set_source(scan)
        c.set_target(moved)

        def state():
            a = c.icp_align(max_corr=3.0, force_iterations=6)
            gi, gd = c.correspondences()
            o = c.outlier_filter(scan, method=wm.WM_OUTLIER_RADIUS, radius=0.5, min_neighbors=5)
            k = c.iss_keypoints(scan, salient_radius=1.0, non_max_radius=0.5, third=True)
            f = c.fpfh(1, counts=True)
            return (a["T"].tobytes(), a["iterations"], a["mse"], host(gi).tobytes(), host(gd).tobytes(), host(o["indices"]).tobytes(),
                    host(o["counts"]).tobytes(), host(k["indices"]).tobytes(), host(k["third"]).tobytes(), f["fpfh"].tobytes(),
                    f["counts"].tobytes())

        before = state()
        nrm = check_normals(wm, c.normals_radius(scan, rn, counts=True, sums=True), scan, rn, RR.normal_reference("scan", 6))
        check_fpfh(c.fpfh_radius(scan, rf, normal_radius=rn, counts=True), scan, nrm, rf, what="between registrations")
        assert state() == before
    finally:
        c.close()


# ------------------------------------------------------------------ the pipeline
PIPE_RADIUS = 1.5  # chosen among 0.5 / 1.0 / 1.5 m with the CPU checkers alone: 79 / 206 / 222 reciprocal matches


def test_keypoints_radius_descriptors_matches_pose_then_icp_on_the_scan(wm):
    """tests/test_iss_gpu.py's four stages on the 6 000-point scan and the scan moved by 40 degrees of yaw and (0.8, 0.6,
    0), with wm_fpfh_radius descriptors (feature radius 1.5 m, normal radius 0.75 m) and NO cloud set on the context for
    them: descriptors of all points, keypoints of both clouds (radii 1.0, 0.5), the keypoints' rows matched, the pose
    from the matches.  The CPU checkers give 225 keypoints on each side (the same points), 222 reciprocal matches, all
    right (206 with 203 right at 1.0 m, 79 with 72 right at 0.5 m), and a refitted pose 1.3e-8 m / < 1e-8 rad from the
    true one."""
    import torch
    import corr_ransac_reference as CR
    from golden_checks import pose_err
    src = np.array(FR.clouds()["scan"])
    T = np.eye(4)
    T[:3, :3] = CR.rotation((0, 0, 1), math.radians(40.0))
    T[:3, 3] = (0.8, 0.6, 0.0)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    c = wm.Context(0)
    try:
        dsrc, dtgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        dev_s = torch.empty((len(src), 33), dtype=torch.float32, device="cuda:0")
        dev_t = torch.empty((len(tgt), 33), dtype=torch.float32, device="cuda:0")
        assert c.fpfh_radius(dsrc, PIPE_RADIUS, normal_radius=PIPE_RADIUS / 2, out=dev_s)["rc"] == 0
        assert c.fpfh_radius(dtgt, PIPE_RADIUS, normal_radius=PIPE_RADIUS / 2, out=dev_t)["rc"] == 0
        ks = c.iss_keypoints(dsrc, salient_radius=1.0, non_max_radius=0.5)
        kt = c.iss_keypoints(dtgt, salient_radius=1.0, non_max_radius=0.5)
        assert np.array_equal(host(ks["indices"]), IR.reference("scan-1.0")["indices"]) and ks["n_out"] == 225
        fs, ft = c.gather_records(dev_s, ks["indices"]), c.gather_records(dev_t, kt["indices"])
        m = c.feature_match(fs, ft, reciprocal=True)
        found = m["idx"] >= 0
        assert m["n_matched"] == int(found.sum()) > 100
        query = ks["indices"][found].contiguous()                      # the source keypoints that found a match
        match = kt["indices"][m["idx"][found].long()].contiguous()     # ... and their targets, as rows of the cloud
        got = c.corr_ransac(dsrc, dtgt, match, query, refine_model=1)
        assert got["rc"] == wm.WM_OK and got["refined"] == 1
        mi, qi = host(match), host(query)
        ref = CR.solve(src, tgt, mi, qi, refine=True, min_d2=got["min_d2"])
        for k in ("n_valid", "iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model", "refined"):
            assert got[k] == ref[k], k
        assert np.array_equal(got["model"].view(np.uint32), ref["model"].view(np.uint32))
        dt, da = pose_err(got["T"], T)
        print("coarse pose: %.2e m, %.2e rad from the true one; %d keypoints, %d matches (%d right), %d kept" %
              (dt, da, ks["n_out"], m["n_matched"], int((mi == qi).sum()), got["n_out"]))
        a = c.icp_match(c.transform_cloud(src, got["T"]), tgt, max_corr=3.0)
        b = c.icp_match(c.transform_cloud(src, T), tgt, max_corr=3.0)
        assert a["rc"] == wm.WM_OK and b["rc"] == wm.WM_OK
        dt, da = pose_err(a["T"] @ got["T"], b["T"] @ T)
        assert dt <= 1e-4 and da <= 1e-4, (dt, da)
    finally:
        c.close()
