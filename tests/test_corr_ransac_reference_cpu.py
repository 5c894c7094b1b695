"""tests/corr_ransac_reference.py held to itself, without a device: the library's host evaluation of the hypothesis rule
(wm.corr_hypothesis) against a float64 numpy.linalg.svd restatement of Umeyama, the sample test and the skips, the
clamp of the automatic sample distance, the loop on counts made up here, and a planted case that shows the rule finds
a pose.

The bound of the hypothesis: both sides end in one rounding to float32 (2^-24 relative each); the float64 work in
front of it differs by ~1e-13 on a well-spread sample (smallest singular-value gap >= 1e-3 of the largest), which can
move a value across a rounding boundary: 4 * 2^-23 * max(1, |entry|) covers both roundings with room."""
import math

import numpy as np
import pytest

import corr_ransac_reference as CR

F = np.float32
BOUND = 4 * 2.0 ** -23


def _samples(n, seed, noise=0.01, scale=10.0, offset=0.0):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        p = (rng.uniform(-scale, scale, (3, 3)) + offset).astype(F)
        R = CR.rotation(rng.normal(size=3), rng.uniform(0, math.pi))
        q = (p.astype(np.float64) @ R.T + rng.uniform(-5, 5, 3) + rng.normal(size=(3, 3)) * noise).astype(F)
        yield p, q


def test_the_rule_on_the_host_equals_the_float64_restatement(wm):
    checked = 0
    for p, q in _samples(3000, 11):
        a, b = CR.hypothesis_lib(p, q, 0.0), CR.hypothesis_svd(p, q, 0.0)
        assert (a is None) == (b is None)
        if a is None:
            continue
        Tb, S = b
        if min(S[0] - S[1], S[1] - S[2]) < 1e-3 * S[0]:
            continue
        checked += 1
        err = np.abs(a.astype(np.float64) - Tb.astype(np.float64))
        assert np.all(err <= BOUND * np.maximum(1.0, np.abs(Tb))), (p, q, a, Tb)
        # a rotation, and the sample is mapped onto its targets to the noise
        R = a[:, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 8 * 2.0 ** -23 and np.linalg.det(R) > 0
    assert checked >= 2500


def test_a_reflected_sample_still_gives_a_rotation(wm):
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    q = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0]], F)  # (a mirror image in the plane: a half turn about x maps it)
    a, b = CR.hypothesis_lib(p, q, 0.0), CR.hypothesis_svd(p, q, 0.0)
    assert np.linalg.det(a[:, :3].astype(np.float64)) > 0.999
    assert np.abs(a.astype(np.float64) - b[0]).max() <= BOUND


DEGENERATE = {
    "duplicate": ([[1, 2, 3], [1, 2, 3], [4, 5, 6]], 0.0),
    "all_equal": ([[1, 2, 3], [1, 2, 3], [1, 2, 3]], 0.0),
    "collinear": ([[0, 0, 0], [1, 1, 1], [2, 2, 2]], 0.0),
    "nan": ([[0, 0, 0], [float("nan"), 0, 0], [0, 1, 0]], 0.0),
    "inf": ([[0, 0, 0], [float("inf"), 0, 0], [0, 1, 0]], 0.0),
    "overflow": ([[0, 0, 0], [3e19, 0, 0], [0, 3e19, 0]], 0.0),
    "underflow": ([[0, 0, 0], [1e-12, 0, 0], [0, 1e-12, 0]], 0.0),
    "too_close_01": ([[0, 0, 0], [0.5, 0, 0], [0, 3, 0]], 1.0),
    "too_close_12": ([[0, 0, 0], [3, 0, 0], [3, 0.5, 0]], 1.0),
    "equal_to_bound": ([[0, 0, 0], [1, 0, 0], [0, 3, 0]], 1.0),  # (d2 == min_d2 fails: the test is >)
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_skipped_samples_are_skipped_by_both(wm, name):
    p, min_d2 = DEGENERATE[name]
    p = np.array(p, F)
    q = (p + F(1)).astype(F)
    flag, T = wm.corr_hypothesis(p, q, min_d2)
    assert flag == 0 and not T.any()
    assert CR.hypothesis_svd(p, q, min_d2) is None and not CR.sample_good(p, min_d2)


def test_the_sample_test_matches_on_a_sweep_of_bounds(wm):
    rng = np.random.default_rng(5)
    skipped = 0
    for _ in range(2000):
        p = rng.uniform(-1, 1, (3, 3)).astype(F)
        q = rng.uniform(-1, 1, (3, 3)).astype(F)
        if rng.random() < 0.2:  # exactly at the bound
            min_d2 = float(CR._d2(p[0], p[1]))
        else:
            min_d2 = float(F(rng.uniform(0, 2)))
        flag, _ = wm.corr_hypothesis(p, q, min_d2)
        assert bool(flag) == CR.sample_good(p, min_d2)
        skipped += not flag
    assert 400 < skipped < 1800


def test_the_automatic_sample_distance_and_its_clamp():
    rng = np.random.default_rng(3)
    P = rng.uniform(-5, 5, (500, 3)).astype(F)
    lam = np.linalg.eigvalsh(np.cov(P.astype(np.float64).T, bias=True))
    want = (np.sqrt(lam).sum() / 3) ** 2
    assert abs(float(CR.min_d2_auto(P)) - want) <= 1e-6 * want
    # a planar cloud: the smallest eigenvalue is zero to rounding and may come out negative; it is clamped, never NaN
    flat = P.copy()
    flat[:, 2] = F(0.7)
    lam2 = np.linalg.eigvalsh(np.cov(flat[:, :2].astype(np.float64).T, bias=True))
    got = float(CR.min_d2_auto(flat))
    assert np.isfinite(got) and abs(got - (np.sqrt(lam2).sum() / 3) ** 2) <= 1e-6 * got
    assert float(CR.min_d2_auto(np.repeat(P[:1], 50, axis=0))) == 0.0
    # the same cloud 1e5 m away: the sums are relative to the first point
    far = (P.astype(np.float64) + 1e5).astype(F)
    lam3 = np.linalg.eigvalsh(np.cov(far.astype(np.float64).T, bias=True))
    assert abs(float(CR.min_d2_auto(far)) - (np.sqrt(lam3).sum() / 3) ** 2) <= 1e-6 * want
    bad = P.copy()
    bad[3, 1] = np.inf
    assert float(CR.min_d2_auto(bad)) == 0.0


def test_the_loop_on_made_up_counts():
    n = 100
    # the third entry counts every pair: k drops below the iterations done and the loop ends behind it
    out = CR.walk_counts([1, 1, 1, 1], [10, 5, 100, 100], n)
    assert out == dict(iterations=3, skipped=0, hypotheses=3, best_hypothesis=2, n_inliers_model=100)
    # an equal count never replaces the best; up to max_iterations + 1 entries are evaluated
    out = CR.walk_counts([1] * 10, [7] * 10, 1000, max_it=4)
    assert out == dict(iterations=5, skipped=0, hypotheses=5, best_hypothesis=0, n_inliers_model=7)
    # skipped entries are no iterations; ten times max_iterations of them end the loop without a model
    out = CR.walk_counts([0] * 60, [0] * 60, n, max_it=5)
    assert out == dict(iterations=0, skipped=50, hypotheses=50, best_hypothesis=-1, n_inliers_model=0)
    out = CR.walk_counts([0, 1, 0, 1, 1], [0, 0, 0, 3, 100], n)
    assert out == dict(iterations=3, skipped=2, hypotheses=5, best_hypothesis=4, n_inliers_model=100)
    # a count of zero is a model (it beats "nothing yet"), and k stays beyond reach
    out = CR.walk_counts([1] * 8, [0] * 8, n, max_it=6)
    assert out == dict(iterations=7, skipped=0, hypotheses=7, best_hypothesis=0, n_inliers_model=0)
    # the stopping rule itself: with w = 0.5, k = log(0.01) / log(1 - 0.125) = 34.5: 35 iterations
    out = CR.walk_counts([1] * 100, [50] * 100, n)
    assert out["iterations"] == 35 and out["hypotheses"] == 35


def test_pairs_of_drops_every_invalid_entry():
    src = np.arange(30, dtype=F).reshape(10, 3)
    tgt = src + F(1)
    src[4, 1] = np.nan
    tgt[7, 0] = np.inf
    mi = np.array([0, -1, 2, 10, 4, 5, -7, 7, 8, 9], np.int32)
    P, Q, e = CR.pairs_of(src, tgt, mi)
    assert e.tolist() == [0, 2, 5, 8, 9]
    qi = np.array([9, 9, 3, 0, 11, -1, 2, 1, 4, 0], np.int32)
    P, Q, e = CR.pairs_of(src, tgt, mi, qi)
    assert e.tolist() == [0, 2, 9]
    assert np.array_equal(P, src[[9, 3, 0]]) and np.array_equal(Q, tgt[[0, 2, 9]])


def test_a_planted_pose_is_found(wm):
    """2 000 pairs, 30 % inliers of a 40 degree rotation about (1, 2, 3) with 2 m of translation and noise <= thr / 4,
    the rest uniform outliers in the box; max_iterations 1000, seed 0."""
    thr = 0.05
    src, tgt, mi, good, T = CR.planted(2000, 0.3, thr, seed=0)
    out = CR.solve(src, tgt, mi, thr=thr, max_it=1000, seed=0)
    assert out["status"] == CR.OK
    got = np.zeros(len(mi), bool)
    got[out["inliers"]] = True
    assert (got & good).sum() >= 0.95 * good.sum()
    wrong = np.nonzero(got & ~good)[0]
    img = src[wrong].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.all(np.linalg.norm(img - tgt[wrong], axis=1) <= thr)
    assert np.array_equal(out["labels"] == CR.INLIER, got) and not (out["labels"] == CR.NONE).any()
    # the refit over those inliers is closer to the planted pose than the three-pair model
    ref = CR.solve(src, tgt, mi, thr=thr, max_it=1000, seed=0, refine=True)
    err = lambda M: np.abs(np.asarray(M, np.float64)[:3] - T[:3]).max()  # noqa: E731
    assert ref["refined"] == 1 and err(ref["T"]) < err(out["T"]) and err(ref["T"]) < 2e-3
