"""GPU parity of the GICP path (k-NN covariances, Mahalanobis matrices, objective /
gradient reduction, BFGS driver) vs the oracle, on the reference's own test cases
(wave_matching/tests/gicp_tests.cpp:43-100).
The same path on stress cases, against the oracle and a numpy reference: tests/test_gicp_stress_gpu.py (cases and
reference: tests/gicp_reference.py, itself checked by tests/test_gicp_reference_cpu.py)."""
import numpy as np
import pytest

from helpers import TOL_R, TOL_T, pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu

# The objective of the minimisations comes in two forms (include/wavematch.h: wm_gicp_params::objective): the opt-in,
# 74 sufficient statistics formed once per outer iteration (csrc/wm_gicp_quad.hpp), and PCL's per-pair sums through the
# float transform.  The oracle restates both (oracle/gicp.c: wmo_gicp_set_objective); the HIP path is held to each
# BIT FOR BIT.  How far the two objectives' registrations are apart: tests/test_gicp_quad_gpu.py.
OBJECTIVES = [("statistics", 1, 1), ("pcl_sums", 0, 0)]   # (name, wm_gicp_params::objective, oracle objective mode)


@pytest.fixture(params=OBJECTIVES, ids=[o[0] for o in OBJECTIVES])
def objective(request, oracle):
    name, hip, orc = request.param
    oracle.gicp_set_objective(orc)
    yield hip
    oracle.gicp_set_objective(0)


# one value per neighbour-list instantiation of k_gicp_cov (8, 10, 12, 16, 20, 24, 32) + edges
@pytest.mark.parametrize("k", [3, 8, 10, 11, 16, 20, 23, 32])
def test_gicp_covariances_match_oracle(wm, ctx, oracle, k):
    ref, tgt, _ = synth.pair(8000 if k > 20 else 20000, seed=4)
    ctx.set_source(ref)
    ctx.set_target(tgt)
    cs, ct = ctx.gicp_covariances(k=k, eps=1e-3)
    ocs = oracle.gicp_covariances(ref, k=k, eps=1e-3)
    oct_ = oracle.gicp_covariances(tgt, k=k, eps=1e-3)
    # same neighbours (exact k-NN, (d2, index) order), same sums, and the same one-sided Jacobi SVD
    # stated with IEEE operations in the same order on both sides (wm_math.hpp svd3<false> /
    # oracle/linalg.c wmo_svd3_jacobi): the matrices are BIT-identical
    for got, want in ((cs, ocs), (ct, oct_)):
        assert np.array_equal(got, want), float(np.abs(got - want).max())
        ev = np.linalg.eigvalsh(got[:200])
        np.testing.assert_allclose(ev, np.tile([1e-3, 1, 1], (200, 1)), atol=1e-9)


def test_gicp_covariances_with_nonfinite_target_points(wm, ctx, oracle):
    """Target covariances are computed in the search grid's own order when every target point is
    finite and in caller order otherwise (non-finite points are not in the grid): both routes must
    give the finite points the oracle's matrices, addressed by CALLER index."""
    ref, tgt, _ = synth.pair(12000, seed=9)
    bad = np.array([0, 17, 4000, 11999])
    tgt_nan = tgt.copy()
    tgt_nan[bad] = np.nan
    keep = np.ones(len(tgt), bool)
    keep[bad] = False
    want = oracle.gicp_covariances(tgt[keep], k=10, eps=1e-3)
    ctx.set_source(ref)
    ctx.set_target(tgt_nan)
    _, ct = ctx.gicp_covariances(k=10, eps=1e-3)
    assert np.array_equal(ct[keep], want)
    # and the all-finite route (grid order) on the same finite points
    ctx.set_target(tgt[keep])
    _, ct2 = ctx.gicp_covariances(k=10, eps=1e-3)
    assert np.array_equal(ct2, ct[keep])


CASES = [("fullResNullMatch", -1.0, 0.0), ("nullDisplacement", 0.05, 0.0),
         ("smallDisplacement", 0.05, 0.2)]


@pytest.mark.parametrize("name,res,tx", CASES)
def test_reference_gicp_cases(wm, ctx, oracle, testscan, objective, name, res, tx):
    P = np.eye(4)
    P[0, 3] = tx
    target = oracle.transform_cloud_d(testscan, P)
    got = ctx.gicp_match(testscan, target, res=res, objective=objective)     # GICPMatcherParams defaults
    a = testscan if res < 0 else oracle.voxel_grid(testscan, res)
    b = target if res < 0 else oracle.voxel_grid(target, res)
    want = oracle.gicp_align(a, b)
    assert got["rc"] == 0 and got["converged"] and want["converged"]
    assert np.linalg.norm(got["T"] - P) < 0.1            # gicp_tests.cpp:36 threshold
    assert got["n_corr"] == want["n_corr"]
    # every sum of the objective is order-independent (double-double) and every other operation is
    # IEEE in the same order on both sides: the two paths take the same decisions throughout
    assert got["iterations"] == want["iterations"] and got["inner_total"] == want["inner_total"]
    assert np.array_equal(got["T"], want["T"])


def test_gicp_objective_and_gradient_match_oracle(wm, ctx, oracle):
    """One fdf evaluation: same pairs, same Mahalanobis matrices, f and gradient to 1e-9."""
    ref, tgt, _ = synth.pair(30000, seed=21)
    ctx.set_source(ref)
    ctx.set_target(tgt)
    T_pair = synth.make_T((0.1, -0.05, 0.02), (0.004, -0.01, 0.015)).astype(np.float32).astype(np.float64)
    x = np.array([0.12, -0.06, 0.03, 0.005, -0.012, 0.017])
    f, g, m = ctx.gicp_eval(T_pair, x, objective=wm.WM_GICP_OBJECTIVE_PCL_SUMS)
    gi, gd = ctx.correspondences()
    moved = oracle.transform_cloud_f(ref, T_pair.astype(np.float32))
    oi, od = oracle.KdTree(tgt).nn(moved)
    keep = od.astype(np.float64) < 25.0
    assert m == keep.sum() and np.array_equal(gi, np.where(keep, oi, -1))
    C1 = oracle.gicp_covariances(ref)
    C2 = oracle.gicp_covariances(tgt)
    R = T_pair[:3, :3]
    M = np.zeros((len(ref), 3, 3))
    si = np.nonzero(keep)[0].astype(np.int32)
    M[si] = np.linalg.inv(C2[oi[si]] + R @ C1[si] @ R.T)
    of, og = oracle.gicp_fdf(ref, tgt, si, oi[si], M, np.eye(4), x)
    assert abs(f - of) <= 1e-12 * abs(of)   # (M through numpy's inverse here: last-bit differences in the terms)
    np.testing.assert_allclose(g, og, rtol=1e-10, atol=1e-10 * np.abs(og).max())
    # ... and the statistics objective (opt-in): the 74 sums of the same pairs, found under T_pair, evaluated at x
    f2, g2, m2 = ctx.gicp_eval(T_pair, x, objective=wm.WM_GICP_OBJECTIVE_STATISTICS)
    qf, qg, Q = oracle.gicp_fdf_statistics(ref, tgt, si, oi[si], M, np.eye(4), T_pair.astype(np.float32), x)
    assert m2 == m and Q[73] == m
    assert abs(f2 - qf) <= 1e-12 * abs(qf)
    np.testing.assert_allclose(g2, qg, rtol=1e-10, atol=1e-10 * np.abs(qg).max())
    # the two objectives are the same function up to the float rounding of PCL's per-point transform (away from the
    # pairing transform): a relative 1e-6 of f at most on 30 000 pairs
    assert abs(f2 - f) <= 3e-6 * abs(f)
    np.testing.assert_allclose(g2, g, rtol=0, atol=3e-5 * np.abs(g).max())
    # at the pairing transform itself the statistics' constant term IS PCL's sum
    x0 = np.array([T_pair[0, 3], T_pair[1, 3], T_pair[2, 3], np.arctan2(np.float32(T_pair[2, 1]), np.float32(T_pair[2, 2])),
                   np.arcsin(-np.float32(T_pair[2, 0])), np.arctan2(np.float32(T_pair[1, 0]), np.float32(T_pair[0, 0]))])
    fa, _, _ = ctx.gicp_eval(T_pair, x0, objective=wm.WM_GICP_OBJECTIVE_PCL_SUMS)
    fb, _, _ = ctx.gicp_eval(T_pair, x0, objective=wm.WM_GICP_OBJECTIVE_STATISTICS)
    assert abs(fa - fb) <= 2e-5 * abs(fa)   # (x0 -> float matrix reproduces T_pair to an ulp or two of its entries)


def test_gicp_on_noisy_synthetic_pair(wm, ctx, oracle, objective):
    """BASELINE config 3 shape (resample pair with noise), small enough for the oracle.
    PCL's inner optimiser (BFGS, gradient tolerance 1e-2, objective evaluated through a
    float-quantised transform) stops wherever its line search lands, so a last-bit difference in f
    or the gradient used to move the result by millimetres (round 1: 3e-3 m vs the oracle).  Now the
    objective's sums are order-independent (double-double accumulation on both sides) and the
    covariances come from the same IEEE-only Jacobi SVD: the HIP path and the oracle make the same
    evaluations (scripts/dev/dev_gicp_trace.py: 113 of 113 identical in hex) and return the same
    float matrix.  north_star's bar is 1e-4 m / 1e-4 rad; asserted here: identical."""
    for n, seed in ((30000, 21), (20000, 7), (40000, 5)):
        ref, tgt, T_gt = synth.pair(n, seed=seed)
        ctx.set_source(ref)
        ctx.set_target(tgt)
        got = ctx.gicp_align(objective=objective)
        want = oracle.gicp_align(ref, tgt)
        assert got["rc"] == 0 and got["converged"] and want["converged"]
        assert got["n_corr"] == want["n_corr"]
        assert got["iterations"] == want["iterations"] and got["inner_total"] == want["inner_total"]
        assert got["evaluations"] == want["evaluations"]
        assert got["f"] == want["f"]
        assert np.array_equal(got["T"], want["T"])
        dt, ang = pose_error(got["T"], T_gt)
        assert dt < 5e-3 and ang < 1e-3


def test_gicp_too_few_points(wm, ctx):
    pts = synth.scene(1000, seed=1)
    ctx.set_source(pts[:5])           # fewer points than corr_rand = 10
    ctx.set_target(pts)
    r = ctx.gicp_align()
    assert r["rc"] == wm.WM_NOT_CONVERGED and r["T"] is None


@pytest.mark.parametrize("name,res,tx", CASES)
def test_reference_gicp_cases_against_pcl_literal_summation(wm, ctx, oracle, testscan, name, res, tx):
    """The oracle's objective can also be summed as PCL / Eigen do it -- plain doubles in index order
    (oracle/gicp.c: wmo_gicp_set_summation(1)) -- instead of the order-independent double-double sums
    the HIP path is held to bit for bit.  On the reference's own cases (gicp_tests.cpp) the HIP path
    stays within north_star's 1e-4 m / 1e-4 rad of that PCL-literal oracle."""
    P = np.eye(4)
    P[0, 3] = tx
    target = oracle.transform_cloud_d(testscan, P)
    got = ctx.gicp_match(testscan, target, res=res, objective=wm.WM_GICP_OBJECTIVE_PCL_SUMS)
    a = testscan if res < 0 else oracle.voxel_grid(testscan, res)
    b = target if res < 0 else oracle.voxel_grid(target, res)
    oracle.gicp_set_summation(1)
    try:
        want = oracle.gicp_align(a, b)
    finally:
        oracle.gicp_set_summation(0)
    assert got["rc"] == 0 and want["converged"]
    dt, ang = pose_error(got["T"], want["T"])
    assert dt <= 1e-4 and ang <= 1e-4, (dt, ang)


def test_gicp_spread_against_pcl_literal_summation(wm, ctx, oracle):
    """On noisy pairs PCL's BFGS (gradient tolerance 1e-2, float-quantised transform) stops wherever its
    line search lands: the last bit of a sum can move the stopping point.  This is the distance between
    the HIP path (= the double-double oracle, bit for bit) and the PCL-literal oracle -- i.e. how far
    ANY faithful implementation may sit from real PCL on such data; both are equally far from ground
    truth.  Reported, and bounded at the millimetre level."""
    rows = []
    for n, seed in ((30000, 21), (20000, 7), (40000, 5)):
        ref, tgt, T_gt = synth.pair(n, seed=seed)
        ctx.set_source(ref)
        ctx.set_target(tgt)
        got = ctx.gicp_align(objective=wm.WM_GICP_OBJECTIVE_PCL_SUMS)
        oracle.gicp_set_summation(1)
        try:
            lit = oracle.gicp_align(ref, tgt)
        finally:
            oracle.gicp_set_summation(0)
        assert got["rc"] == 0 and lit["converged"]
        dt, ang = pose_error(got["T"], lit["T"])
        dg, ag = pose_error(got["T"], T_gt)
        dl, al = pose_error(lit["T"], T_gt)
        rows.append((n, seed, dt, ang, dg, dl, got["inner_total"], lit["inner_total"]))
        assert dt < 5e-3 and ang < 1e-3
        assert abs(dg - dl) < 5e-3      # neither summation is closer to the truth in any systematic way
    for r in rows:
        print("GICP %d pts seed %d: HIP vs PCL-literal oracle %.2e m / %.2e rad | vs ground truth: HIP %.2e m, "
              "literal %.2e m | inner iterations %d vs %d" % r)


def _gicp_run(wm, ref, tgt, served, **kw):
    # (the resident evaluator serves the PER-PAIR objective; the default -- sufficient statistics -- needs none)
    kw.setdefault("objective", wm.WM_GICP_OBJECTIVE_PCL_SUMS)
    c = wm.Context(0)
    try:
        c.set_option("gicp_served", served)
        c.set_source(ref)
        c.set_target(tgt)
        return c.gicp_align(**kw)
    finally:
        c.close()


def test_served_evaluations_give_the_launched_ones_bits(wm):
    """The resident evaluator (k_gicp_fdf_served: trial points through a mailbox in device memory,
    answers through pinned slots) and a kernel launch per evaluation run the same arithmetic in the
    same order: same matrix, same objective, same number of evaluations -- on the reference-sized
    case and on a noisy pair where a last-bit difference would move the BFGS stopping point."""
    for n, seed, mode in ((20000, 3, "resample"), (40000, 9, "copy")):
        ref, tgt, _ = synth.pair(n, seed=seed, mode=mode)
        a = _gicp_run(wm, ref, tgt, 0)
        b = _gicp_run(wm, ref, tgt, 1)
        assert a["rc"] == b["rc"] == 0
        assert a["served_evaluations"] == 0
        assert b["served_evaluations"] == b["evaluations"] > 0, "the evaluator was not used (no large BAR here?)"
        assert a["evaluations"] == b["evaluations"] and a["iterations"] == b["iterations"]
        assert a["f"] == b["f"]
        assert np.array_equal(a["T"], b["T"])


def test_concurrent_registrations_share_the_evaluator_budget(wm):
    """Registrations running at once on one GPU (a MultiMatcher's workers): resident evaluators are admitted
    while their workgroups fit the device together, the others launch their evaluations meanwhile --
    every one of them gets the same answer."""
    import threading
    ref, tgt, _ = synth.pair(30000, seed=21, mode="resample")
    want = _gicp_run(wm, ref, tgt, 0)
    out = [None] * 4

    def work(k):
        for _ in range(3):
            out[k] = _gicp_run(wm, ref, tgt, 1)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r in out:
        assert r is not None and r["rc"] == 0
        assert np.array_equal(r["T"], want["T"]) and r["f"] == want["f"]


def test_served_evaluator_gives_up_and_the_host_recovers(wm):
    """A host that stalls for longer than the resident evaluator's guard (0.2 s without a command): the
    kernel leaves by itself (it must never hold the GPU waiting for a dead host), the stalled call
    notices, falls back to launching its evaluations -- and the registration's result is the same."""
    ref, tgt, _ = synth.pair(20000, seed=3, mode="resample")
    want = _gicp_run(wm, ref, tgt, 0)
    c = wm.Context(0)
    try:
        c.set_option("gicp_served", 1)
        c.set_option("gicp_serve_test_stall_ms", 350)
        c.set_source(ref)
        c.set_target(tgt)
        got = c.gicp_align(objective=wm.WM_GICP_OBJECTIVE_PCL_SUMS)
        c.set_option("gicp_serve_test_stall_ms", 0)
        again = c.gicp_align(objective=wm.WM_GICP_OBJECTIVE_PCL_SUMS)   # the context is fully usable afterwards, served again
    finally:
        c.close()
    assert got["rc"] == 0 and np.array_equal(got["T"], want["T"]) and got["f"] == want["f"]
    assert 0 < got["served_evaluations"] < got["evaluations"]
    assert again["rc"] == 0 and np.array_equal(again["T"], want["T"])
    assert again["served_evaluations"] == again["evaluations"]


@pytest.mark.parametrize("case", ["tiny", "partial-overlap", "beyond-the-on-chip-copy", "no-copy-variant"])
def test_served_evaluations_corner_cases(wm, case):
    """The resident evaluator against a launch per evaluation where its code paths differ: one
    workgroup only; pairs without a match among the ones kept on chip; more than eight pairs per
    thread (the ninth onwards streamed from HBM behind the on-chip ones); the variant that keeps
    nothing on chip.  Identical matrix, objective and evaluation count every time."""
    served = 1
    kw = {}
    if case == "tiny":
        ref, tgt, _ = synth.pair(300, seed=31, mode="resample")
    elif case == "partial-overlap":
        ref, tgt, _ = synth.pair(30000, seed=32, mode="resample")
        tgt = tgt[tgt[:, 0] < 10.0]          # a good part of the source has nothing within 5 m ... or barely
        kw = dict(max_corr=1.0)
    elif case == "beyond-the-on-chip-copy":
        ref, tgt, _ = synth.pair(600000, seed=33)   # 256 workgroups x 256 threads x 8 pairs = 524 288 < 600 000
    else:
        ref, tgt, _ = synth.pair(50000, seed=34, mode="resample")
        served = 2
    a = _gicp_run(wm, ref, tgt, 0, **kw)
    b = _gicp_run(wm, ref, tgt, served, **kw)
    assert a["rc"] == b["rc"]
    assert a["evaluations"] == b["evaluations"] and a["iterations"] == b["iterations"]
    if a["rc"] == 0:
        assert a["f"] == b["f"] and np.array_equal(a["T"], b["T"])
    if b["evaluations"] > 0:
        assert b["served_evaluations"] == b["evaluations"]
