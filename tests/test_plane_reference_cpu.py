"""The checker of the point-to-plane metric, checked itself (tests/plane_reference.py; no GPU): normals of an exact
plane, the Gauss-Newton step against a finite-difference minimiser of sum (n . (R p + t - q))^2, the iterations to stop
on the issue's pairs, and the reference's own 0.1 threshold on the split-scan pairs."""
import numpy as np
import pytest

import plane_reference as PR
from libwave_amd import synth

YAML = dict(max_corr=3.0, max_iter=100, t_eps=1e-8, fit_eps=1e-2)  # tests/golden/config/icp.yaml


def test_normals_of_an_exact_plane():
    rng = np.random.default_rng(1)
    pts = np.zeros((3000, 3), np.float32)
    pts[:, :2] = rng.uniform(-10, 10, (3000, 2)).astype(np.float32)
    pts[:, 2] = 2.0  # the plane z = 2: seen from the origin its normal points down
    N = PR.normals(pts, 20)
    assert N["valid"].all()
    assert np.abs(N["normal"] - np.array([0.0, 0.0, -1.0])).max() < 1e-12
    assert np.abs(N["curvature"]).max() < 1e-12
    pts[:, 2] = 0.0  # through the origin: n . p = 0, either sign
    N = PR.normals(pts, 20)
    assert np.abs(np.abs(N["normal"]) - np.array([0.0, 0.0, 1.0])).max() < 1e-12
    assert np.abs(N["curvature"]).max() == 0.0
    # the neighbourhood is the k nearest, the point itself first, ties by index
    idx, d2 = PR.knn(pts, 20)
    assert np.array_equal(idx[:, 0], np.arange(len(pts))) and (d2[:, 0] == 0).all()
    assert (np.diff(d2.astype(np.float64), axis=1) >= 0).all()
    brute = np.linalg.norm(pts[7].astype(np.float64) - pts.astype(np.float64), axis=1)
    assert set(idx[7, :20]) == set(np.argsort(brute, kind="stable")[:20])


def test_non_finite_points_and_coincident_neighbourhoods_give_zeros():
    pts = synth.scene(2000, seed=5).copy()
    pts[3] = np.nan
    pts[50:80] = np.float32([200.0, -150.0, 30.0])
    N = PR.normals(pts, 20)
    assert not N["valid"][3] and not N["valid"][50:80].any()
    assert np.array_equal(N["normal"][3], np.zeros(3)) and not N["normal"][50:80].any()
    assert N["valid"].sum() == len(pts) - 31


def _objective(x, p, q, n):
    R = PR.rodrigues(x[3:])
    return float(((((p @ R.T) + x[:3] - q) * n).sum(1) ** 2).sum())


def test_step_against_a_finite_difference_minimiser(oracle):
    """With the pairs held fixed, repeated steps (each linearised at the pose it starts from) and a Newton iteration on
    central differences of the objective itself must arrive at the same transform: both stop where the gradient of
    sum (n . (R p + t - q))^2 vanishes.  h = 1e-4 puts the difference quotients' zero within O(h^2) = 1e-8 of the true
    one; the bar is 1e-6."""
    ref, tgt, _ = synth.pair(4000, seed=11, mode="resample")
    nrm = PR.normals(tgt, 20)["normal"]
    idx, d2 = oracle.KdTree(tgt).nn(ref)
    p, q, n = ref.astype(np.float64), tgt[idx].astype(np.float64), nrm[idx]
    T = np.eye(4)
    first = None
    for _ in range(12):
        cur = p @ T[:3, :3].T + T[:3, 3]
        st = PR.plane_sums(cur, q, n, d2)
        assert not PR.degenerate(st)
        Tk = PR.step(st)
        first = Tk if first is None else first
        T = Tk @ T
    assert np.linalg.norm(Tk - np.eye(4)) < 1e-12  # (arrived)
    h = 1e-4
    E = np.eye(6) * h
    x = np.zeros(6)
    f = lambda y: _objective(y, p, q, n)  # noqa: E731
    for _ in range(8):
        g = np.array([(f(x + E[a]) - f(x - E[a])) / (2 * h) for a in range(6)])
        H = np.zeros((6, 6))
        for a in range(6):
            for b in range(a, 6):
                H[a, b] = H[b, a] = (f(x + E[a] + E[b]) - f(x + E[a] - E[b]) - f(x - E[a] + E[b]) + f(x - E[a] - E[b])) / (4 * h * h)
        x = x + np.linalg.solve(H, -g)
    X = np.eye(4)
    X[:3, :3] = PR.rodrigues(x[3:])
    X[:3, 3] = x[:3]
    assert np.linalg.norm(T - X) < 1e-6, np.linalg.norm(T - X)
    # ... and ONE step already goes most of the way (what makes four iterations enough): it lowers the objective
    x1 = np.zeros(6)
    x1[:3] = first[:3, 3]
    x1[3:] = 0.5 * np.array([first[2, 1] - first[1, 2], first[0, 2] - first[2, 0], first[1, 0] - first[0, 1]])
    assert _objective(x1, p, q, n) < _objective(np.zeros(6), p, q, n)


def test_one_plane_is_degenerate():
    rng = np.random.default_rng(2)
    q = np.zeros((500, 3))
    q[:, :2] = rng.uniform(-5, 5, (500, 2))
    n = np.tile([0.0, 0.0, 1.0], (500, 1))
    st = PR.plane_sums(q + [0.02, 0.01, 0.0], q, n, np.full(500, 5e-4, np.float32))
    assert PR.degenerate(st)
    # two more wall directions constrain every motion
    n2 = n.copy()
    n2[:150] = [1.0, 0.0, 0.0]
    n2[150:300] = [0.0, 1.0, 0.0]
    assert not PR.degenerate(PR.plane_sums(q + [0.02, 0.01, 0.3], q, n2, np.full(500, 5e-4, np.float32)))


# iterations to stop, point-to-point (the oracle's restatement of PCL) and point-to-plane, with the yaml's criteria and
# with fit_eps = 1e-6: the issue's table for the two synthetic pairs; for the split-scan pairs what this restatement
# gives with the pair construction of PR.split_pair
SYNTH_COUNTS = {"uniform": ((13, 4), (31, 8)), "rings": ((11, 4), (26, 8))}


@pytest.mark.parametrize("pattern", ["uniform", "rings"])
def test_stop_iterations_on_the_synthetic_pairs(oracle, pattern):
    ref, tgt, _ = synth.pair(20000, mode="resample", pattern=pattern)
    nrm = PR.normals(tgt, 20)
    assert ((nrm["gap"] < 1e-3) | nrm["tie"]).mean() <= 0.03
    for fit_eps, (want_point, want_plane) in zip((1e-2, 1e-6), SYNTH_COUNTS[pattern]):
        point = oracle.icp_align(ref, tgt, incremental_float=0, **dict(YAML, fit_eps=fit_eps))
        plane = PR.align(oracle, ref, tgt, tgt_normals=nrm["normal"], **dict(YAML, fit_eps=fit_eps))
        assert plane["converged"] and plane["margin"] > 1e-6
        assert (point["iterations"], plane["iterations"]) == (want_point, want_plane)


SPLIT_COUNTS = [((5, 5), (10, 9)), ((9, 4), (11, 10)), ((12, 7), (16, 11))]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_split_scan_pairs_stop_sooner_and_stay_within_the_reference_threshold(oracle, testscan, case):
    tt, yaw, pitch = PR.SPLIT_PERTURBATIONS[case]
    ref, tgt, T_gt = PR.split_pair(oracle, testscan, tt, yaw, pitch)
    nrm = PR.normals(tgt, 20)
    assert ((nrm["gap"] < 1e-3) | nrm["tie"]).mean() <= 0.03
    for fit_eps, (want_point, want_plane) in zip((1e-2, 1e-6), SPLIT_COUNTS[case]):
        point = oracle.icp_align(ref, tgt, incremental_float=0, **dict(YAML, fit_eps=fit_eps))
        plane = PR.align(oracle, ref, tgt, tgt_normals=nrm["normal"], **dict(YAML, fit_eps=fit_eps))
        assert plane["converged"] and plane["margin"] > 1e-6
        assert np.linalg.norm(plane["T"] - T_gt) < 0.1  # the reference's own threshold (icp_tests.cpp:38)
        assert plane["iterations"] <= point["iterations"]
        assert (point["iterations"], plane["iterations"]) == (want_point, want_plane)
