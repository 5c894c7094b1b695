"""wm_iss_keypoints and wm_gather_records (libwave_amd/csrc/wm_iss.hip) on the GPU against tests/iss_reference.py.

Everything is held by EQUALITY to the checker: the keypoints' indices, n_out, the labels, the neighbour counts, the
three counters, and `third` bit for bit -- the scatter sums are integers, and the saliency step is IEEE double on both
sides.  tests/test_iss_reference_cpu.py holds the checker's two forms to each other on every case used here, and the
rule to PCL's own arithmetic."""
import math

import numpy as np
import pytest

import iss_reference as IR

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def dev(wm):
    c = wm.Context(0)
    yield c
    c.close()


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(got, ref, what="", rc=0):
    assert got["rc"] == rc, what
    assert np.array_equal(host(got["indices"]), ref["indices"]), what
    assert got["n_out"] == len(ref["indices"]) == got["n_keypoints"] == ref["n_keypoints"], what
    assert (got["n_finite"], got["n_salient"]) == (ref["n_finite"], ref["n_salient"]), what
    assert np.array_equal(host(got["labels"]), ref["labels"]), what
    assert np.array_equal(host(got["counts"]), ref["counts"]), what
    assert host(got["third"]).tobytes() == ref["third"].tobytes(), what


def run(dev, cloud, rs, rn, **kw):
    return dev.iss_keypoints(cloud, salient_radius=rs, non_max_radius=rn, third=True, counts=True, **kw)


def key(g):
    return (g["rc"], g["n_out"], host(g["indices"]).tobytes(), host(g["labels"]).tobytes(), host(g["third"]).tobytes(),
            host(g["counts"]).tobytes(), g["n_finite"], g["n_salient"], g["n_keypoints"])


# ------------------------------------------------------------------ the base cases
@pytest.mark.parametrize("name", ["scene-1.0", "scene-6x", "rings-1.0", "rings-6x", "scan-1.0", "scan-6x"])
def test_base_cases_equal_the_checker(dev, name):
    c, rs, rn = IR.base_cases()[name]
    same(run(dev, np.array(c), rs, rn), IR.reference(name), name)


def test_the_large_scene_equals_the_checker(dev):
    cloud, ref = IR.big_case()
    got = run(dev, cloud, *IR.BIG_RADII)
    same(got, ref, "scene 20000")
    assert (got["n_salient"], got["n_keypoints"]) == (15503, 654)


def test_sizes_around_the_wave(dev):
    d = IR.dense_cloud(193)
    for n in list(range(1, 66)) + [193]:
        same(run(dev, d[:n], 1.0, 0.6), IR.keypoints(d[:n], 1.0, 0.6), "n = %d" % n)


# ------------------------------------------------------------------ degenerate clouds, radii, parameters
@pytest.mark.parametrize("name", ["nan-inf", "all-nan", "duplicate", "far", "whole-cloud-nms", "lattice", "gamma-0",
                                  "min-neighbors-high", "all-salient-kept"])
def test_variants_equal_the_checker(dev, name):
    c, rs, rn, kw = IR.variants()[name]
    ref = IR.keypoints(c, rs, rn, **kw)
    got = run(dev, np.array(c), rs, rn, **kw)
    same(got, ref, name)
    if name == "all-nan":
        assert got["n_finite"] == 0 and got["n_out"] == 0 and not host(got["labels"]).any()
        assert np.all(host(got["counts"]) == -1)
    if name == "nan-inf":
        bad = ~np.isfinite(c).all(1)
        assert bad.sum() > 300 and np.all(host(got["labels"])[bad] == IR.NONE) and got["n_keypoints"] > 0
    if name == "duplicate":
        k, n = host(got["indices"]), len(c) // 2
        assert len(k) > 4 and np.array_equal(k[:len(k) // 2] + n, k[len(k) // 2:])
    if name == "whole-cloud-nms":  # one keypoint survives a suppression over the whole cloud: the largest third
        assert got["n_keypoints"] == 1 and host(got["indices"])[0] == int(np.argmax(ref["third"]))
    if name in ("lattice", "gamma-0", "min-neighbors-high"):
        assert got["n_salient"] == 0 and got["n_keypoints"] == 0
    if name == "all-salient-kept":
        assert got["n_keypoints"] == got["n_salient"] > 100


def test_a_pair_at_exactly_r2_is_out_and_one_ulp_below_is_in(dev):
    at = np.array([[0, 0, 0], [0.5, 0, 0]], F)
    below = np.array([[0, 0, 0], [np.nextafter(F(0.5), F(0)), 0, 0]], F)
    assert list(host(run(dev, at, 0.5, 0.5, min_neighbors=0)["counts"])) == [1, 1]
    assert list(host(run(dev, below, 0.5, 0.5, min_neighbors=0)["counts"])) == [2, 2]


# ------------------------------------------------------------------ order and position
def test_row_permutations_give_the_same_keypoints(dev):
    c, rs, rn = IR.base_cases()["scan-1.0"]
    ref = IR.reference("scan-1.0")
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(len(c))
        got = run(dev, np.ascontiguousarray(c[perm]), rs, rn)
        assert np.array_equal(np.sort(perm[host(got["indices"])]), ref["indices"])
        assert host(got["third"]).tobytes() == ref["third"][perm].tobytes()
        assert np.array_equal(host(got["labels"]), ref["labels"][perm])
        assert np.array_equal(host(got["counts"]), ref["counts"][perm])


# ------------------------------------------------------------------ options and memory
def test_the_cell_size_changes_no_byte(dev, wm):
    c, rs, rn = IR.base_cases()["rings-6x"]
    ref = IR.reference("rings-6x")
    try:
        for div in (0.5, 2.0, 8.0):
            dev.set_option("iss_cell_div", div)
            same(run(dev, np.array(c), rs, rn), ref, "iss_cell_div %g" % div)
        with pytest.raises(wm.WmError):
            dev.set_option("iss_cell_div", 0.25)
    finally:
        dev.set_option("iss_cell_div", 2.0)


def test_memory_spaces_strides_cap_and_repeatability(dev, wm):
    import torch
    c, rs, rn = IR.base_cases()["scan-1.0"]
    c = np.array(c)
    ref = IR.reference("scan-1.0")
    base = run(dev, c, rs, rn)
    same(base, ref, "host 12")
    assert key(run(dev, c, rs, rn)) == key(base)  # two calls: identical bytes

    def wide(a, w):
        out = np.full((len(a), w), 7.5, F)
        out[:, :3] = a
        return out

    assert key(run(dev, wide(c, 4), rs, rn)) == key(base)
    for w in (3, 4, 8):  # strides 12, 16, 32 in device memory; 32 in host memory through a CPU tensor
        d = torch.from_numpy(wide(c, w)).cuda()
        got = run(dev, d, rs, rn)
        assert got["indices"].is_cuda and got["labels"].is_cuda and got["third"].is_cuda and got["counts"].is_cuda
        assert key(got) == key(base)
        got = run(dev, d, rs, rn, out_mem=wm.WM_MEM_HOST)
        assert isinstance(got["indices"], np.ndarray) and key(got) == key(base)
    got = run(dev, torch.from_numpy(wide(c, 8)), rs, rn, out_mem=wm.WM_MEM_DEVICE)
    assert got["indices"].is_cuda and key(got) == key(base)
    # no optional output at all
    got = dev.iss_keypoints(c, salient_radius=rs, non_max_radius=rn, labels=False)
    assert got["labels"] is None and got["third"] is None and got["counts"] is None
    assert np.array_equal(got["indices"], ref["indices"]) and got["n_salient"] == ref["n_salient"]
    # cap one short: WM_ERR_ARG, the true n_out, the first cap entries
    cap = base["n_out"] - 1
    got = run(dev, c, rs, rn, cap=cap)
    assert got["rc"] == wm.WM_ERR_ARG and got["n_out"] == base["n_out"]
    assert np.array_equal(got["indices"], ref["indices"][:cap]) and np.array_equal(got["labels"], ref["labels"])
    got = run(dev, torch.from_numpy(c).cuda(), rs, rn, cap=cap)
    assert got["rc"] == wm.WM_ERR_ARG and got["n_out"] == base["n_out"]
    assert np.array_equal(host(got["indices"]), ref["indices"][:cap])


# ------------------------------------------------------------------ state
def test_the_registration_state_and_the_other_workspaces_are_untouched(wm):
    import fpfh_reference as FR
    scan = np.ascontiguousarray(FR.clouds()["scan"])
    moved = (scan.astype(np.float64) + [0.3, 0.1, 0.0]).astype(F)
    c = wm.Context(0)
    try:
        c.set_source(scan)
        c.set_target(moved)

        def state():
            a = c.icp_align(max_corr=3.0, force_iterations=6)
            gi, gd = c.correspondences()
            o = c.outlier_filter(scan, method=wm.WM_OUTLIER_RADIUS, radius=0.5, min_neighbors=5)
            k = c.cluster_extract(scan, tolerance=0.5, min_cluster_size=5)
            return (a["T"].tobytes(), a["iterations"], a["mse"], host(gi).tobytes(), host(gd).tobytes(), host(o["indices"]).tobytes(),
                    host(o["counts"]).tobytes(), host(k["indices"]).tobytes(), host(k["labels"]).tobytes())

        before = state()
        got = run(c, scan, 1.0, 0.5)
        same(got, IR.reference("scan-1.0"), "between registrations")
        idx = np.arange(0, 6000, 7, dtype=np.int32)
        assert np.array_equal(c.gather_records(scan, idx), scan[idx])
        assert state() == before
    finally:
        c.close()


# ------------------------------------------------------------------ wm_gather_records
@pytest.mark.parametrize("width", [33, 36])  # strides 132 and 144
def test_gather_records(dev, wm, width):
    import torch
    rng = np.random.default_rng(5)
    src = rng.normal(size=(700, width)).astype(F)
    dsrc = torch.from_numpy(src).cuda()
    for m in (0, 1, 63, 64, 65, 1000):
        idx = rng.integers(0, 700, m).astype(np.int32)  # with repeats
        if m >= 63:
            idx[5] = idx[40] = 699
            idx[0] = 0
        got = dev.gather_records(src, idx)
        assert got.shape == (m, width) and got.tobytes() == src[idx].tobytes()
        got = dev.gather_records(dsrc, torch.from_numpy(idx).cuda())
        assert got.is_cuda and got.cpu().numpy().tobytes() == src[idx].tobytes()
    for bad in (700, -1, 2 ** 31 - 1):
        idx = np.array([3, 5, bad, 7], np.int32)
        with pytest.raises(wm.WmError):
            dev.gather_records(src, idx)
        with pytest.raises(wm.WmError):
            dev.gather_records(dsrc, torch.from_numpy(idx).cuda())
    # the call after a refused one is clean
    idx = np.arange(10, dtype=np.int32)
    assert dev.gather_records(dsrc, torch.from_numpy(idx).cuda()).cpu().numpy().tobytes() == src[:10].tobytes()


# ------------------------------------------------------------------ the pipeline
def test_keypoints_descriptors_matches_pose_then_icp_on_the_scan(wm):
    """The four stages on the 6 000-point scan and the scan moved by 40 degrees of yaw and (0.8, 0.6, 0), radii (1.0,
    0.5): descriptors of all points, keypoints of both clouds, the keypoints' rows matched, the pose from the matches.
    The CPU checkers give 225 keypoints on each side (the same points), 216 reciprocal matches, all right, and a
    refitted pose 1.2e-8 m / 4.2e-8 rad from the true one."""
    import torch
    import corr_ransac_reference as CR
    import fpfh_reference as FR
    from golden_checks import pose_err
    src = np.array(FR.clouds()["scan"])
    T = np.eye(4)
    T[:3, :3] = CR.rotation((0, 0, 1), math.radians(40.0))
    T[:3, 3] = (0.8, 0.6, 0.0)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    c = wm.Context(0)
    try:
        c.set_source(src)
        c.set_target(tgt)
        dsrc, dtgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        dev_s = torch.empty((len(src), 33), dtype=torch.float32, device="cuda:0")
        dev_t = torch.empty((len(tgt), 33), dtype=torch.float32, device="cuda:0")
        assert c.fpfh(0, out=dev_s)["rc"] == 0 and c.fpfh(1, out=dev_t)["rc"] == 0
        ks = run(c, dsrc, 1.0, 0.5)
        kt = run(c, dtgt, 1.0, 0.5)
        same(ks, IR.reference("scan-1.0"), "source keypoints")
        same(kt, IR.keypoints(tgt, 1.0, 0.5), "target keypoints")
        assert ks["n_out"] == 225
        fs, ft = c.gather_records(dev_s, ks["indices"]), c.gather_records(dev_t, kt["indices"])
        assert fs.cpu().numpy().tobytes() == dev_s.cpu().numpy()[host(ks["indices"])].tobytes()
        m = c.feature_match(fs, ft, reciprocal=True)
        found = m["idx"] >= 0
        assert m["n_matched"] == int(found.sum()) > 100
        query = ks["indices"][found].contiguous()                      # the source keypoints that found a match
        match = kt["indices"][m["idx"][found].long()].contiguous()     # ... and their targets, as rows of the cloud
        got = c.corr_ransac(dsrc, dtgt, match, query, refine_model=1)
        assert got["rc"] == wm.WM_OK and got["refined"] == 1
        # the device's result equals the checker's on those correspondences
        mi, qi = host(match), host(query)
        P, Q, e = CR.pairs_of(src, tgt, mi, qi)
        ref = CR.solve(src, tgt, mi, qi, refine=True, min_d2=got["min_d2"])
        for k in ("n_valid", "iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model", "refined"):
            assert got[k] == ref[k], k
        assert np.array_equal(got["model"].view(np.uint32), ref["model"].view(np.uint32))
        dt, da = pose_err(got["T"], T)
        print("coarse pose: %.2e m, %.2e rad from the true one; %d keypoints, %d matches, %d kept" %
              (dt, da, ks["n_out"], m["n_matched"], got["n_out"]))
        a = c.icp_match(c.transform_cloud(src, got["T"]), tgt, max_corr=3.0)
        b = c.icp_match(c.transform_cloud(src, T), tgt, max_corr=3.0)
        assert a["rc"] == wm.WM_OK and b["rc"] == wm.WM_OK
        dt, da = pose_err(a["T"] @ got["T"], b["T"] @ T)
        assert dt <= 1e-4 and da <= 1e-4, (dt, da)
    finally:
        c.close()
