"""wm_corr_ransac (libwave_amd/csrc/wm_corr_ransac.hip) on the GPU against tests/corr_ransac_reference.py.

The hypotheses the device evaluates are bit-equal to the library's host evaluation of the same rule (wm.corr_hypothesis),
skips included; the loop's counters, the model's bits, the inliers and the labels equal the checker's on the same
inputs.  With the automatic sample distance the checker applies the bound the device reports (stats min_d2), after
that bound has been held to the checker's own float64 value: the device adds the nine sums exactly, numpy does not, and
a bound that differs in its last bit could flip a sample test."""
import ctypes as C
import math

import numpy as np
import pytest

import corr_ransac_reference as CR
import sac_reference as SR

pytestmark = pytest.mark.gpu

F = np.float32
BOUND = 4 * 2.0 ** -23
TILE = 1024  # kCorrTile: pairs of a count workgroup's tile


@pytest.fixture(scope="module")
def dev(wm):
    c = wm.Context(0)
    yield c
    c.close()


def same(got, ref, what=""):
    assert got["rc"] == ref["status"], what
    for k in ("n_valid", "iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model", "refined"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    if ref["status"] != CR.OK:
        assert got["T"] is None and got["n_out"] == 0 and len(got["inliers"]) == 0
        return
    assert np.array_equal(got["model"].view(np.uint32), ref["model"].view(np.uint32)), what
    assert np.array_equal(np.asarray(got["inliers"]), ref["inliers"]), what
    assert np.array_equal(np.asarray(got["labels"]), ref["labels"]), what
    assert got["n_out"] == len(ref["inliers"]) == got["n_inliers"]
    if not ref["refined"]:
        want = np.eye(4)
        want[:3] = ref["model"].astype(np.float64)
        assert np.array_equal(got["T"], want), what


def check(dev, src, tgt, mi, qi=None, what="", **kw):
    """the device's call and the checker's on the same inputs -> the device's dict"""
    got = dev.corr_ransac(src, tgt, mi, qi, **kw)
    P, _, _ = CR.pairs_of(src, tgt, mi, qi)
    auto = kw.get("min_sample_distance", -1.0) < 0
    if got["n_valid"] >= 3:
        if auto:
            want = float(CR.min_d2_auto(P))
            assert abs(float(got["min_d2"]) - want) <= 1e-5 * want + 1e-30, (got["min_d2"], want)
        else:
            assert got["min_d2"] == CR.min_d2_given(kw["min_sample_distance"])
    ref = CR.solve(src, tgt, mi, qi, thr=kw.get("inlier_threshold", 0.05), max_it=kw.get("max_iterations", 1000),
                   prob=kw.get("probability", 0.99), seed=kw.get("seed", 0), refine=False,
                   min_d2=got["min_d2"] if got["n_valid"] >= 3 else 0.0)
    if kw.get("refine_model"):  # the model's part here; the refit has its own test
        for k in ("n_valid", "iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model"):
            assert got[k] == ref[k], (what, k)
        if ref["status"] == CR.OK:
            assert np.array_equal(got["model"].view(np.uint32), ref["model"].view(np.uint32)), what
    else:
        same(got, ref, what)
    return got


# ------------------------------------------------------------------ hypotheses
@pytest.mark.parametrize("min_dist", [-1.0, 0.0, 9.0])
def test_hypotheses_are_bit_equal_to_the_host_rule(dev, wm, min_dist):
    src, tgt, mi, good, T = CR.planted(700, 0.4, 0.05, seed=3)
    src[5] = src[9]  # duplicates and a collinear triple among the source points: skipped entries
    src[11] = src[9]
    got = dev.corr_ransac(src, tgt, mi, max_iterations=5, min_sample_distance=min_dist)
    P, Q, e = CR.pairs_of(src, tgt, mi)
    Td, fl = dev.debug_corr_hypotheses(0, 600)
    skipped = 0
    for j in range(600):
        i = list(SR.sample(0, j, len(P)))
        flag, Th = wm.corr_hypothesis(P[i], Q[i], got["min_d2"])
        assert fl[j] == flag, j
        assert np.array_equal(Td[j].view(np.uint32), Th.view(np.uint32)), (j, Td[j], Th)
        skipped += not flag
    assert (skipped > 150) == (min_dist > 0)
    # another window of the stream, and a far seed
    got = dev.corr_ransac(src, tgt, mi, max_iterations=5, min_sample_distance=0.0, seed=2 ** 63 + 11)
    Td, fl = dev.debug_corr_hypotheses(10 ** 12, 64)
    for j in range(64):
        i = list(SR.sample(2 ** 63 + 11, 10 ** 12 + j, len(P)))
        flag, Th = wm.corr_hypothesis(P[i], Q[i], 0.0)
        assert fl[j] == flag and np.array_equal(Td[j].view(np.uint32), Th.view(np.uint32))


def test_hypotheses_far_from_the_origin(dev, wm):
    src, tgt, mi, good, T = CR.planted(300, 0.5, 0.2, seed=4, offset=1.0e5)
    got = dev.corr_ransac(src, tgt, mi, max_iterations=5, inlier_threshold=0.2)
    Td, fl = dev.debug_corr_hypotheses(0, 256)
    for j in range(256):
        i = list(SR.sample(0, j, 300))
        flag, Th = wm.corr_hypothesis(src[i], tgt[i], got["min_d2"])
        assert fl[j] == flag and np.array_equal(Td[j].view(np.uint32), Th.view(np.uint32)), j


# ------------------------------------------------------------------ counts, loop, selection: sizes
@pytest.mark.parametrize("mv", [3, 4, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_sizes_around_every_boundary(dev, mv):
    src, tgt, mi, good, T = CR.planted(mv, 0.5, 0.05, seed=mv)
    check(dev, src, tgt, mi, what="mv %d" % mv, max_iterations=60)


@pytest.mark.parametrize("where", ["head", "tail", "every_second"])
def test_entries_without_a_match(dev, where):
    src, tgt, mi, good, T = CR.planted(700, 0.5, 0.05, seed=8)
    mi = mi.copy()
    if where == "head":
        mi[:130] = -1
    elif where == "tail":
        mi[-131:] = -1
    else:
        mi[::2] = -1
    got = check(dev, src, tgt, mi, what=where, max_iterations=60)
    assert got["n_valid"] == int((mi >= 0).sum()) and np.all(np.asarray(got["labels"])[mi < 0] == CR.NONE)


def test_bad_indices_and_non_finite_points(dev):
    src, tgt, mi, good, T = CR.planted(600, 0.5, 0.05, seed=9)
    mi = mi.copy()
    mi[3], mi[77], mi[300], mi[599] = 600, -5, 2 ** 31 - 1, -2 ** 31
    src[10, 0], src[11, 2], tgt[12, 1], tgt[13, 0], tgt[14, 2] = np.nan, np.inf, np.nan, -np.inf, np.inf
    got = check(dev, src, tgt, mi, what="bad", max_iterations=60)
    assert got["n_valid"] == 600 - 9
    assert np.all(np.asarray(got["labels"])[[3, 77, 300, 599, 10, 11, 12, 13, 14]] == CR.NONE)
    # the source side through query_idx: out of range on either side of it
    qi = np.arange(600, dtype=np.int32)
    qi[20], qi[21] = -1, 600
    got = check(dev, src, tgt, mi, qi, what="bad query", max_iterations=60)
    assert got["n_valid"] == 600 - 11


def test_query_idx_as_a_permutation_with_repeats(dev):
    src, tgt, mi, good, T = CR.planted(500, 0.5, 0.05, seed=10)
    rng = np.random.default_rng(10)
    perm = rng.permutation(500).astype(np.int32)
    check(dev, src, tgt, perm.copy(), perm, what="permutation", max_iterations=60)  # entry e pairs perm[e] with perm[e]
    qi = np.r_[perm, perm[:100]].astype(np.int32)  # a hundred source points matched twice: counted once per entry
    got = check(dev, src, tgt, qi.copy(), qi, what="repeats", max_iterations=60)
    assert got["n_valid"] == 600
    lab = np.asarray(got["labels"])
    assert np.array_equal(lab[:100], lab[500:])


# ------------------------------------------------------------------ rounds
@pytest.fixture(scope="module")
def round_case():
    src, tgt, mi, good, T = CR.planted(1000, 0.3, 0.05, seed=12)
    refs = {it: CR.solve(src, tgt, mi, max_it=it, min_sample_distance=9.0) for it in (1, 2, 50, 1000)}
    return src, tgt, mi, refs


@pytest.mark.parametrize("R", [1, 7, 256, 1024])
def test_how_the_stream_is_cut_changes_only_rounds(dev, wm, round_case, R):
    src, tgt, mi, refs = round_case
    dev.set_option("corr_round", R)
    try:
        for it, ref in refs.items():
            got = dev.corr_ransac(src, tgt, mi, max_iterations=it, min_sample_distance=9.0)
            same(got, ref, "corr_round %d max_iterations %d" % (R, it))
            hyp = got["hypotheses"]
            assert got["rounds"] >= -(-hyp // R) and (got["rounds"] == hyp if R == 1 else got["rounds"] <= max(hyp, 1))
    finally:
        dev.set_option("corr_round", 256)
    ref = refs[1000]
    assert 0.3 < ref["skipped"] / ref["hypotheses"] < 0.7  # (the sample distance skips roughly half the entries)
    for bad in (0, 1025, -1):
        with pytest.raises(wm.WmError):
            dev.set_option("corr_round", bad)


def test_all_entries_skipped_is_no_model(dev, wm):
    src, tgt, mi, good, T = CR.planted(300, 0.5, 0.05, seed=13)
    src[:] = src[0]
    got = dev.corr_ransac(src, tgt, mi, max_iterations=20)
    assert got["rc"] == wm.WM_NOT_CONVERGED and got["T"] is None and got["n_out"] == 0 and got["labels"] is None
    assert (got["iterations"], got["skipped"], got["hypotheses"], got["best_hypothesis"]) == (0, 200, 200, -1)
    assert got["n_valid"] == 300 and got["min_d2"] == 0.0
    # fewer than three valid entries among many, in device memory: no model either
    import torch
    mi2 = np.full(300, -1, np.int32)
    mi2[[5, 250]] = 7
    got = dev.corr_ransac(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(mi2).cuda())
    assert got["rc"] == wm.WM_NOT_CONVERGED and got["n_valid"] == 2 and got["hypotheses"] == 0


# ------------------------------------------------------------------ refit
def _refit_check(dev, src, tgt, mi, thr, what):
    got = dev.corr_ransac(src, tgt, mi, inlier_threshold=thr, refine_model=1)
    P, Q, e = CR.pairs_of(src, tgt, mi)
    ref = CR.solve(src, tgt, mi, thr=thr, refine=True, min_d2=got["min_d2"])
    for k in ("iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model", "refined"):
        assert got[k] == ref[k], (what, k)
    assert np.array_equal(got["model"].view(np.uint32), ref["model"].view(np.uint32))
    # the inliers: the checker's selection from the RETURNED transform's float rounding
    inl, lab = CR.select(P, Q, e, len(mi), got["T"], thr)
    assert np.array_equal(got["inliers"], inl) and np.array_equal(got["labels"], lab) and got["n_out"] == len(inl)
    # T_out against the float64 Umeyama over the model's inliers
    err = np.abs(got["T"][:3] - ref["T"][:3])
    assert np.all(err <= BOUND * np.maximum(1.0, np.abs(ref["T"][:3]))), (what, err.max())
    assert np.array_equal(got["T"][3], [0, 0, 0, 1])
    return got


def test_refit(dev):
    src, tgt, mi, good, T = CR.planted(3000, 0.3, 0.05, seed=14)
    got = _refit_check(dev, src, tgt, mi, 0.05, "refit")
    assert got["refined"] == 1 and got["n_inliers"] >= 0.95 * good.sum()
    assert np.abs(got["T"][:3] - T[:3]).max() < 2e-3
    mi = mi.copy()
    mi[::3] = -1
    _refit_check(dev, src, tgt, mi, 0.05, "refit with holes")


def test_refit_far_from_the_origin(dev):
    """1e5 m on both clouds: a float there has steps of 8 mm, so the threshold is 0.2; the sums relative to the winning
    sample's first pair are what lets the refit keep float64's precision."""
    src, tgt, mi, good, T = CR.planted(2000, 0.4, 0.2, seed=15, offset=1.0e5)
    got = _refit_check(dev, src, tgt, mi, 0.2, "far")
    assert got["refined"] == 1 and got["n_inliers"] >= 0.9 * good.sum()
    R = got["T"][:3, :3]
    assert np.abs(R - T[:3, :3]).max() < 1e-3 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12


def test_fewer_than_three_inliers_keep_the_model(dev):
    rng = np.random.default_rng(16)
    src = rng.uniform(-10, 10, (200, 3)).astype(F)
    tgt = rng.uniform(-10, 10, (200, 3)).astype(F)
    mi = np.arange(200, dtype=np.int32)
    got = dev.corr_ransac(src, tgt, mi, inlier_threshold=1e-4, max_iterations=30, refine_model=1)
    ref = CR.solve(src, tgt, mi, thr=1e-4, max_it=30, min_d2=got["min_d2"])
    assert ref["n_inliers_model"] < 3
    same(got, ref, "no refit")


# ------------------------------------------------------------------ memory
def test_memory_spaces_strides_cap_and_repeatability(dev, wm):
    import torch
    src, tgt, mi, good, T = CR.planted(900, 0.4, 0.05, seed=17)
    mi = mi.copy()
    mi[::7] = -1
    base = check(dev, src, tgt, mi, what="host 12", max_iterations=100, refine_model=0)
    key = lambda g: (g["rc"], g["T"].tobytes(), np.asarray(g["inliers"]).tobytes(), np.asarray(g["labels"]).tobytes(),  # noqa: E731
                     g["model"].tobytes(), g["iterations"], g["hypotheses"], g["n_out"])
    assert key(dev.corr_ransac(src, tgt, mi, max_iterations=100)) == key(base)  # two calls: identical bytes

    def wide(a, w):
        out = np.full((len(a), w), 7.5, F)
        out[:, :3] = a
        return out

    def host(g):
        return dict(g, inliers=g["inliers"].cpu().numpy() if hasattr(g["inliers"], "cpu") else g["inliers"],
                    labels=g["labels"].cpu().numpy() if hasattr(g["labels"], "cpu") else g["labels"])

    assert key(dev.corr_ransac(wide(src, 4), wide(tgt, 4), mi, max_iterations=100)) == key(base)
    for w in (3, 4, 8):  # strides 12, 16, 32 in device memory; 32 in host memory through a CPU tensor
        ds, dt = torch.from_numpy(wide(src, w)).cuda(), torch.from_numpy(wide(tgt, w)).cuda()
        got = dev.corr_ransac(ds, dt, torch.from_numpy(mi).cuda(), max_iterations=100)
        assert got["inliers"].is_cuda and got["labels"].is_cuda
        assert key(host(got)) == key(base)
        got = dev.corr_ransac(ds, dt, torch.from_numpy(mi).cuda(), max_iterations=100, out_mem=wm.WM_MEM_HOST)
        assert isinstance(got["inliers"], np.ndarray) and key(got) == key(base)
    got = dev.corr_ransac(torch.from_numpy(wide(src, 8)), torch.from_numpy(wide(tgt, 8)), mi, max_iterations=100,
                          out_mem=wm.WM_MEM_DEVICE)
    assert got["inliers"].is_cuda and key(host(got)) == key(base)
    # query_idx in device memory
    qi = np.arange(900, dtype=np.int32)
    got = dev.corr_ransac(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(mi).cuda(),
                          torch.from_numpy(qi).cuda(), max_iterations=100)
    assert key(host(got)) == key(base)
    # cap smaller than the count: WM_ERR_ARG, the true n_out, the first cap entries
    cap = base["n_out"] // 2
    got = dev.corr_ransac(src, tgt, mi, max_iterations=100, cap=cap)
    assert got["rc"] == wm.WM_ERR_ARG and got["n_out"] == base["n_out"]
    assert np.array_equal(got["inliers"], base["inliers"][:cap]) and np.array_equal(got["labels"], base["labels"])
    got = dev.corr_ransac(src, tgt, mi, max_iterations=100, cap=0, labels=False)
    assert got["rc"] == wm.WM_ERR_ARG and got["n_out"] == base["n_out"] and got["labels"] is None


def test_the_registration_state_is_untouched(dev, wm):
    import fpfh_reference as FR
    scan = np.ascontiguousarray(FR.clouds()["scan"])
    moved = (scan.astype(np.float64) + [0.3, 0.1, 0.0]).astype(F)
    c = wm.Context(0)
    try:
        c.set_source(scan)
        c.set_target(moved)
        a = c.icp_align(max_corr=3.0, force_iterations=6)
        src, tgt, mi, good, T = CR.planted(1500, 0.3, 0.05, seed=18)
        assert c.corr_ransac(src, tgt, mi, refine_model=1)["rc"] == wm.WM_OK
        b = c.icp_align(max_corr=3.0, force_iterations=6)
        assert a["T"].tobytes() == b["T"].tobytes() and a["iterations"] == b["iterations"] and a["mse"] == b["mse"]
    finally:
        c.close()


# ------------------------------------------------------------------ the pipeline
def test_descriptors_matches_pose_then_icp_on_the_scan(dev, wm):
    """Target = 6 000 points of the scan fixture moved by 40 degrees of yaw and 1 m (0.8, 0.6, 0).  Chosen on the CPU
    first (fpfh_reference on plane_reference's normals and lists, fpfh_reference.match, this checker, oracle.icp_align):
    40 degrees, the largest of 10 / 20 / 40, satisfies every assertion below there -- 5 484 reciprocal matches, 5 455 of
    them right, a coarse pose 2.1e-5 m / 4.3e-7 rad from the true one, and both ICP runs at the same pose to 1.4e-8 m."""
    import torch
    import fpfh_reference as FR
    from golden_checks import pose_err
    src = np.array(FR.clouds()["scan"])  # (a writable copy: it goes to the device through torch)
    T = np.eye(4)
    T[:3, :3] = CR.rotation((0, 0, 1), math.radians(40.0))
    T[:3, 3] = (0.8, 0.6, 0.0)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    c = wm.Context(0)
    try:
        c.set_source(src)
        c.set_target(tgt)
        dev_s = torch.empty((len(src), 33), dtype=torch.float32, device="cuda:0")
        dev_t = torch.empty((len(tgt), 33), dtype=torch.float32, device="cuda:0")
        assert c.fpfh(0, out=dev_s)["rc"] == 0 and c.fpfh(1, out=dev_t)["rc"] == 0
        m = c.feature_match(dev_s, dev_t, reciprocal=True)
        assert m["idx"].is_cuda and m["n_matched"] > 1000
        got = c.corr_ransac(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), m["idx"], refine_model=1)
        assert got["rc"] == wm.WM_OK and got["refined"] == 1
        # the device's result equals the checker's on those correspondences
        mi = m["idx"].cpu().numpy()
        P, Q, e = CR.pairs_of(src, tgt, mi)
        ref = CR.solve(src, tgt, mi, refine=True, min_d2=got["min_d2"])
        for k in ("n_valid", "iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model", "refined"):
            assert got[k] == ref[k], k
        assert np.array_equal(got["model"].view(np.uint32), ref["model"].view(np.uint32))
        inl, lab = CR.select(P, Q, e, len(mi), got["T"], 0.05)
        assert np.array_equal(got["inliers"].cpu().numpy(), inl) and np.array_equal(got["labels"].cpu().numpy(), lab)
        assert np.all(np.abs(got["T"][:3] - ref["T"][:3]) <= BOUND * np.maximum(1.0, np.abs(ref["T"][:3])))
        dt, da = pose_err(got["T"], T)
        print("coarse pose: %.2e m, %.2e rad from the true one; %d of %d matches kept" % (dt, da, got["n_out"], got["n_valid"]))
        # the matchers start from identity: the pose is applied to the source, then ICP
        a = c.icp_match(c.transform_cloud(src, got["T"]), tgt, max_corr=3.0)
        b = c.icp_match(c.transform_cloud(src, T), tgt, max_corr=3.0)
        assert a["rc"] == wm.WM_OK and b["rc"] == wm.WM_OK
        dt, da = pose_err(a["T"] @ got["T"], b["T"] @ T)
        assert dt <= 1e-4 and da <= 1e-4, (dt, da)
    finally:
        c.close()
