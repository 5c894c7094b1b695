"""The device's information estimators (k_lum_sums / k_lum_ss / k_censi, libwave_amd/csrc/wm_info.hip)
where test_info_gpu.py does not reach: registrations that converge at rotated poses on either branch of
Eigen's eulerAngles(0, 1, 2), result poses an align from identity cannot reach (yaw 2.5 rad, the gimbal,
roll near pi), more source points than one grid-stride step covers (kInfoBlocks x kBlock = 131 072),
queries without a match, LUMold searching with its own max_corr, points where the spherical Jacobian is
singular, and clouds 5.6e4 m from the origin.

Every case gives the estimators the KERNEL's own correspondences (ctx.correspondences()) and compares the
device against both the oracle's literal restatement (oracle/info.c) and the independent float64
restatement (tests/info_reference.py), so that the estimator is tested apart from the registration."""
import math

import numpy as np
import pytest

import info_reference as IR
from helpers import pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu

REL = 1e-7                      # H and M: the reference's float sub-products (tests/test_info_reference_cpu.py)
LUM_REL = 4.0 * 2.0 ** -24      # s^2 rounded to float, 1 / s^2 in float: the device vs the exact sum of its terms
OFFSET = np.array([12345.0, -54321.0, 250.0], np.float32)


def _align(wm, ctx, ref, tgt, **kw):
    ctx.set_source(ref)
    ctx.set_target(tgt)
    r = ctx.icp_align(max_corr=3.0, nn_method=wm.WM_NN_GRID, **kw)
    assert r["rc"] == 0 and r["converged"], r
    idx, _ = ctx.correspondences()
    ok = idx >= 0
    assert ok.sum() == r["n_corr"]
    return r, ok, idx


def _jittered_copy(n, T, seed=21, sigma=0.002):
    """target = T ref + 2 mm noise: an align from identity lands within 1e-4 of T."""
    ref, tgt, _ = synth.pair(n, seed=seed, mode="copy", T=T)
    tgt = (tgt + np.random.default_rng(seed).normal(0, sigma, tgt.shape)).astype(np.float32)
    return ref, tgt


def _nan_equal_and_close(got, want, tol, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    fin = ~np.isnan(want)
    err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
    assert err <= tol, "%s: max |diff| %.3e > %.3e" % (what, err, tol)


def _check_censi(wm, ctx, oracle, b, a, T):
    rc, got, _ = ctx.icp_info(wm.WM_INFO_CENSI, T_result=T)
    assert rc == 0
    o = oracle.censi_from_pairs(b, a, T)
    r = IR.censi(b, a, T)
    if np.isnan(o["info"]).all():
        assert np.isnan(got).all() and np.isnan(r["M"]).all()
        return got
    tol = IR.info_tolerance(r["H"], r["M"], REL)
    _nan_equal_and_close(got, o["info"], tol, "censi: device vs oracle")
    _nan_equal_and_close(got, r["info"], tol, "censi: device vs f64 restatement")
    return got


def _check_lum(wm, ctx, oracle, ref, tgt, T, ok, idx, rel_extra=0.0):
    """estimateLUM on the align's pairs.  The device sums the reference's float s^2 terms in double and
    rounds once; the reference sums them sequentially in float.  So: the device against the exact sum of
    the same float terms (math.fsum) to LUM_REL, against the oracle to the oracle's own measured error."""
    rc, got, deg = ctx.icp_info(wm.WM_INFO_LUM)
    assert rc == 0 and not deg
    p = oracle.transform_cloud_f(ref[ok], T)
    q = tgt[idx[ok]]
    every = np.arange(len(p))
    o = oracle.lum_from_pairs(p, q)
    exact = IR.lum(p, q, pairs=(every, every), exact_ss=True)
    sc = np.abs(exact["info"]).max()
    np.testing.assert_allclose(got, exact["info"], rtol=LUM_REL + rel_extra, atol=1e-12 * sc)
    float_sum_err = abs(o["ss"] - exact["ss"]) / exact["ss"]
    np.testing.assert_allclose(got, o["info"], rtol=float_sum_err + LUM_REL + rel_extra, atol=1e-12 * sc)
    return float_sum_err


def _check_lumold(wm, ctx, oracle, ref, tgt, T, max_corr, rel_extra=0.0):
    rc, got, _ = ctx.icp_info(wm.WM_INFO_LUMOLD, max_corr=max_corr)
    assert rc == 0
    fin = oracle.transform_cloud_f(ref, T)
    i, j = IR.lumold_pairs(fin, tgt, max_corr)
    o = oracle.lum_from_pairs(fin[i], tgt[j])
    exact = IR.lum(fin, tgt, pairs=(i, j), exact_ss=True)
    sc = np.abs(exact["info"]).max()
    np.testing.assert_allclose(got, exact["info"], rtol=LUM_REL + rel_extra, atol=1e-12 * sc)
    float_sum_err = abs(o["ss"] - exact["ss"]) / exact["ss"]
    np.testing.assert_allclose(got, o["info"], rtol=float_sum_err + LUM_REL + rel_extra, atol=1e-12 * sc)
    return len(i)


@pytest.mark.parametrize("rpy,flip", [((0.05, 0.02, -0.03), False), ((-0.05, 0.02, 0.03), True),
                                      ((0.06, -0.05, 0.08), False), ((-0.08, 0.05, -0.1), True)])
def test_estimators_at_a_converged_rotated_pose(wm, ctx, oracle, rpy, flip):
    T = synth.make_T(t=(0.3, -0.2, 0.1), rpy=rpy)
    ref, tgt = _jittered_copy(30000, T)
    r, ok, idx = _align(wm, ctx, ref, tgt)
    dt, ang = pose_error(r["T"], T)
    assert dt <= 1e-4 and ang <= 1e-4, (dt, ang)
    assert IR.euler_flipped(r["T"][:3, :3]) == flip
    _check_censi(wm, ctx, oracle, ref[ok], tgt[idx[ok]], r["T"])
    _check_lum(wm, ctx, oracle, ref, tgt, r["T"], ok, idx)
    _check_lumold(wm, ctx, oracle, ref, tgt, r["T"], 3.0)


@pytest.mark.parametrize("rpy", [(0.0, 0.0, 2.5), (0.4, -0.3, 0.7), (-0.4, 0.3, -0.7),
                                 (math.pi - 1e-3, 0.1, 0.2), (-math.pi + 1e-3, 0.1, 0.2),
                                 (0.1, math.pi / 2 - 1e-6, 0.2), (0.1, -math.pi / 2 + 1e-6, 0.2)],
                         ids=["yaw2.5", "rpy+", "rpy-", "roll~+pi", "roll~-pi", "pitch~+pi/2", "pitch~-pi/2"])
def test_censi_arithmetic_at_result_poses_an_align_cannot_reach(wm, ctx, oracle, rpy):
    """wm_icp_info takes T_result from the caller (ICPMatcher passes its `result`): after one converged align,
    the Censi arithmetic at poses far from identity, with translations up to 50 m."""
    ref, tgt = _jittered_copy(20000, synth.make_T(t=(0.1, -0.05, 0.02), rpy=(0.01, -0.01, 0.02)))
    r, ok, idx = _align(wm, ctx, ref, tgt)
    for t in ((0.0, 0.0, 0.0), (3.0, -2.0, 1.0), (50.0, -20.0, 5.0)):
        _check_censi(wm, ctx, oracle, ref[ok], tgt[idx[ok]], synth.make_T(t=t, rpy=rpy))


@pytest.mark.parametrize("n", [131071, 131072, 131073, 300001, 1000000])
def test_estimators_past_one_grid_stride(wm, ctx, oracle, n):
    """kInfoBlocks x kBlock = 131 072 pairs per grid-stride step: one short, exact, one over, and two and
    eight steps.  At 1M the reference's sequential float s^2 is itself off; the device is held to the
    exact sum of the same float terms, and to the oracle within that sum's measured error."""
    ref, tgt, _ = synth.pair(n, seed=31, mode="resample")
    r, ok, idx = _align(wm, ctx, ref, tgt)
    assert ok.sum() > 0.9 * n
    _check_censi(wm, ctx, oracle, ref[ok], tgt[idx[ok]], r["T"])
    err = _check_lum(wm, ctx, oracle, ref, tgt, r["T"], ok, idx)
    assert err < 1e-3     # (a sequential float sum of 1M positive terms: measured, not assumed)
    _check_lumold(wm, ctx, oracle, ref, tgt, r["T"], 3.0)


def test_estimators_with_unmatched_queries_and_lumold_radii(wm, ctx, oracle):
    """A third of the source lifted 12 m: no match within the align's 3 m (the kNoIdx skip in all three
    kernels), some within LUMold's 10 m; LUMold searches with max_corr 0.5, 3 and 10 (a resampled target,
    so that some of the align's pairs are farther apart than 0.5 m)."""
    T = synth.make_T(t=(0.3, -0.2, 0.1), rpy=(0.03, -0.02, 0.05))
    ref, tgt, _ = synth.pair(30000, seed=23, mode="resample", T=T)
    far = np.arange(len(ref)) % 3 == 0
    ref = ref.copy()
    ref[far, 2] += 12.0
    r, ok, idx = _align(wm, ctx, ref, tgt)
    assert not ok[far].any() and ok[~far].mean() > 0.99
    _check_censi(wm, ctx, oracle, ref[ok], tgt[idx[ok]], r["T"])
    _check_lum(wm, ctx, oracle, ref, tgt, r["T"], ok, idx)
    kept = {mc: _check_lumold(wm, ctx, oracle, ref, tgt, r["T"], mc) for mc in (0.5, 3.0, 10.0)}
    assert kept[0.5] < kept[3.0] < kept[10.0]
    # the align's own correspondences survive LUMold's private searches
    idx2, _ = ctx.correspondences()
    assert np.array_equal(idx2, idx)


@pytest.mark.parametrize("with_origin", [False, True], ids=["axis_and_cut", "with_origin"])
def test_estimators_at_singular_spherical_jacobian_points(wm, ctx, oracle, with_origin):
    """Matched points on the z axis (atan(+-inf)), on atan2's branch cut (x < 0, y = +-0) and at (0, 0, 0)
    (atan(0 / 0) = NaN, which the reference lets poison the whole Censi matrix): NaN entry for entry as the
    oracle, the finite entries to tolerance; LUM has no trigonometry and stays finite."""
    T = synth.make_T(t=(0.05, -0.03, 0.02), rpy=(0.01, -0.01, 0.02))
    ref, tgt = _jittered_copy(20000, T, seed=25)
    edge = [[0.0, 0.0, 4.0], [0.0, 0.0, -2.0], [-5.0, 0.0, 1.0], [-3.0, -0.0, 2.0]]
    if with_origin:
        edge.append([0.0, 0.0, 0.0])
    edge = np.array(edge, np.float32)
    keep_r = np.min(np.linalg.norm(ref[:, None, :] - edge[None], axis=2), axis=1) > 1.5
    keep_t = np.min(np.linalg.norm(tgt[:, None, :] - edge[None], axis=2), axis=1) > 1.5
    ref, tgt = np.vstack([ref[keep_r], edge]), np.vstack([tgt[keep_t], edge])
    r, ok, idx = _align(wm, ctx, ref, tgt)
    ne = len(edge)
    assert ok[-ne:].all() and np.array_equal(idx[-ne:], np.arange(len(tgt) - ne, len(tgt)))
    got = _check_censi(wm, ctx, oracle, ref[ok], tgt[idx[ok]], r["T"])
    assert np.isnan(got).all() == with_origin
    _check_lum(wm, ctx, oracle, ref, tgt, r["T"], ok, idx)


def test_estimators_far_from_the_origin(wm, ctx, oracle):
    """The pair moved 5.6e4 m out (float resolution there: 4 mm).  H's condition is ~1e13, so the Censi
    matrix the reference forms as (H^-1 M H^-1)^-1 is dominated by its own rounding and is held only to
    info_reference.info_tolerance's bound (which grows with cond(H)^2 cond(M)); LUM's normal equations
    are ill-conditioned too (D moves along their weak direction), measured 2e-6 on s^2."""
    T = synth.make_T(t=(0.1, -0.05, 0.02), rpy=(0.0, 0.0, 0.0))
    ref, tgt = _jittered_copy(30000, T, seed=27, sigma=0.01)
    ref, tgt = (ref + OFFSET).astype(np.float32), (tgt + OFFSET).astype(np.float32)
    r, ok, idx = _align(wm, ctx, ref, tgt)
    assert ok.mean() > 0.99
    _check_censi(wm, ctx, oracle, ref[ok], tgt[idx[ok]], r["T"])
    _check_lum(wm, ctx, oracle, ref, tgt, r["T"], ok, idx, rel_extra=2e-6)
    _check_lumold(wm, ctx, oracle, ref, tgt, r["T"], 3.0, rel_extra=2e-6)
