"""Point-to-plane ICP on the device (WM_ICP_PLANE: k_normals, k_plane_stats, k_plane_solve, libwave_amd/csrc/wm_plane.hip)
against the float64 numpy restatement tests/plane_reference.py: normals, the 29 sums, whole registrations, match()'s
scales, the degenerate case, the estimators after a plane align, the batch route, and that the mode leaves nothing behind.

Bounds: 1e-6 rad / 1e-6 for normals and curvature (float64 covariance, eigen-gap >= 1e-3: rounding gives ~1e-12; the
device stores float32), 1e-12 relative to a block's largest entry for the sums (float64 terms, exact across waves),
helpers.TOL_T / TOL_R for poses.  The largest differences belong in DESIGN.md section 4.7; every test prints its own."""
import ctypes

import numpy as np
import pytest

import plane_reference as PR
from helpers import TOL_R, TOL_T, pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu

YAML = dict(max_corr=3.0, max_iter=100, t_eps=1e-8, fit_eps=1e-2)  # tests/golden/config/icp.yaml


def _pairs(oracle, testscan):
    out = []
    for pat in ("uniform", "rings"):
        r, t, T = synth.pair(20000, mode="resample", pattern=pat)
        out.append((pat, r, t, T))
    for i, (tt, yaw, pitch) in enumerate(PR.SPLIT_PERTURBATIONS):
        r, t, T = PR.split_pair(oracle, testscan, tt, yaw, pitch)
        out.append(("split%d" % i, r, t, T))
    return out


_NORMALS = {}


def _ref_normals(name, tgt):
    """the reference's normals of a pair's target (ten seconds of numpy at 20 000 points: once per session)"""
    if name not in _NORMALS:
        _NORMALS[name] = PR.normals(tgt, PR.DEFAULT_K)["normal"]
    return _NORMALS[name]


_check_normals = PR.check_normals  # (shared with tests/test_knn_stress_gpu.py)


# ------------------------------------------------------------------ 1. normals
@pytest.mark.parametrize("name", ["uniform", "rings", "testscan"])
def test_normals_against_the_reference(wm, ctx, oracle, testscan, name):
    import torch
    if name == "testscan":
        cloud = oracle.voxel_grid(testscan, 0.1)
    else:
        cloud = synth.pair(20000, mode="resample", pattern=name)[1]
    ctx.set_source(cloud)
    ctx.set_target(cloud)
    tgt = ctx.estimate_normals(1, 20)
    _check_normals(tgt, cloud, 20, name + " (target)")
    src = ctx.estimate_normals(0, 20)
    _check_normals(src, cloud, 20, name + " (source)")
    dev = torch.full((len(cloud), 4), 7.0, dtype=torch.float32, device="cuda")
    ctx.estimate_normals(1, 0, out=dev)  # k = 0: the default, 20
    assert np.array_equal(dev.cpu().numpy(), tgt)
    dev0 = torch.full((len(cloud), 4), 7.0, dtype=torch.float32, device="cuda")
    ctx.estimate_normals(0, 20, out=dev0)
    assert np.array_equal(dev0.cpu().numpy(), src)


def test_normals_of_non_finite_points_and_coincident_neighbourhoods_are_zero(wm, ctx):
    cloud = synth.scene(6000, seed=5).copy()
    cloud[10] = np.nan
    cloud[11, 1] = np.inf
    cloud[100:130] = np.float32([200.0, -150.0, 30.0])  # thirty copies of one point, far from everything else
    ctx.set_source(cloud)
    ctx.set_target(cloud)
    for which in (1, 0):
        got = ctx.estimate_normals(which, 20)
        assert np.array_equal(got[[10, 11]], np.zeros((2, 4), np.float32))
        assert np.array_equal(got[100:130], np.zeros((30, 4), np.float32))
        rest = np.ones(len(cloud), bool)
        rest[[10, 11]] = False
        rest[100:130] = False
        assert (np.abs(np.linalg.norm(got[rest, :3], axis=1) - 1.0) < 1e-6).all()
    L = wm.lib()
    buf = np.zeros((len(cloud), 4), np.float32)
    for bad_k in (1, 2, 33, -1):
        assert L.wm_estimate_normals(ctx._h, 1, bad_k, ctypes.c_void_p(buf.ctypes.data), wm.WM_MEM_HOST) == wm.WM_ERR_ARG
    assert L.wm_estimate_normals(ctx._h, 2, 20, ctypes.c_void_p(buf.ctypes.data), wm.WM_MEM_HOST) == wm.WM_ERR_ARG


# ------------------------------------------------------------------ 2. sums
POSES = [np.eye(4), synth.make_T((0.15, -0.1, 0.05), (0.01, -0.02, 0.015)), synth.make_T((-0.3, 0.2, -0.1), (-0.02, 0.01, 0.04))]


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_plane_sums_against_the_reference(wm, ctx, pose):
    ref, tgt, _ = synth.pair(20000, mode="resample")
    T = POSES[pose]
    ctx.set_source(ref)
    ctx.set_target(tgt)
    nrm = ctx.estimate_normals(1, 20)
    ctx.nn_search(T, max_corr=3.0, nn_method=wm.WM_NN_GRID)
    got = ctx.icp_stats_for(T, wm.WM_ICP_PLANE)
    again = ctx.icp_stats_for(T, wm.WM_ICP_PLANE)
    assert got.tobytes() == again.tobytes()
    idx, d2 = ctx.correspondences()
    ok = idx >= 0
    pf = PR.transform_f32(ref, T)
    # (the reference's own sums in extended precision: what is measured is the device's rounding, not numpy's)
    ld = np.longdouble
    p, q, n = pf[ok].astype(ld), tgt[idx[ok]].astype(ld), nrm[idx[ok], :3].astype(ld)
    J = np.concatenate([n, np.cross(p, n)], axis=1)
    r = (n * (p - q)).sum(1)
    H = np.array([[(J[:, a] * J[:, b]).sum() for b in range(6)] for a in range(6)])
    g = np.array([(J[:, a] * r).sum() for a in range(6)])
    assert got[0] == ok.sum() and got[31] == len(ref)
    sd2 = d2[ok].astype(ld).sum()
    assert abs(got[1] - sd2) <= 1e-12 * sd2
    eh = np.abs(got[2:23] - H[np.triu_indices(6)].astype(np.float64)).max() / float(np.abs(H).max())
    eg = np.abs(got[23:29] - g.astype(np.float64)).max() / float(np.abs(g).max())
    print("pose %d: J^T J rel %.3e, J^T r rel %.3e" % (pose, eh, eg))
    assert eh <= 1e-12 and eg <= 1e-12, (eh, eg)
    assert np.array_equal(got[29:31], np.zeros(2))
    # the restatement's float64 sums agree too
    st = PR.plane_sums(pf[ok], tgt[idx[ok]], nrm[idx[ok], :3], d2[ok])
    assert np.abs(st[2:23] - got[2:23]).max() <= 1e-10 * np.abs(st[2:23]).max()
    # a second run of search + sums: the same bits
    ctx.nn_search(T, max_corr=3.0, nn_method=wm.WM_NN_GRID)
    assert ctx.icp_stats_for(T, wm.WM_ICP_PLANE).tobytes() == got.tobytes()


# ------------------------------------------------------------------ 3. whole registrations
@pytest.mark.parametrize("fit_eps", [1e-2, 1e-6])
def test_registrations_against_the_reference(wm, ctx, oracle, testscan, fit_eps):
    worst = (0.0, 0.0)
    for name, ref, tgt, T_gt in _pairs(oracle, testscan):
        want = PR.align(oracle, ref, tgt, tgt_normals=_ref_normals(name, tgt), **dict(YAML, fit_eps=fit_eps))
        assert want["margin"] > 1e-6, (name, want["margin"])  # (else: swap the pair's seed)
        ctx.set_source(ref)
        ctx.set_target(tgt)
        got = ctx.icp_align(mode=wm.WM_ICP_PLANE, carry_state=0, **dict(YAML, fit_eps=fit_eps))
        svd = ctx.icp_align(mode=wm.WM_ICP_SVD, carry_state=0, **dict(YAML, fit_eps=fit_eps))
        again = ctx.icp_align(mode=wm.WM_ICP_PLANE, carry_state=0, **dict(YAML, fit_eps=fit_eps))
        print("%s fit_eps %g: plane %d iterations (%s), reference %d (%s), svd %d" %
              (name, fit_eps, got["iterations"], got["state"], want["iterations"], PR.STATE_NAMES[want["state"]], svd["iterations"]))
        assert got["rc"] == 0 and want["converged"], (name, got)
        assert got["iterations"] == want["iterations"], (name, got["iterations"], want["iterations"])
        assert got["state"] == PR.STATE_NAMES[want["state"]], (name, got["state"])
        assert got["n_corr"] == want["n_corr"]
        dt, ang = pose_error(got["T"], want["T"])
        print("    pose vs reference: %.3e m, %.3e rad" % (dt, ang))
        assert dt <= TOL_T and ang <= TOL_R, (name, dt, ang)
        worst = (max(worst[0], dt), max(worst[1], ang))
        assert got["iterations"] <= svd["iterations"], (name, got["iterations"], svd["iterations"])
        assert np.linalg.norm(got["T"] - T_gt) < 0.1
        assert again["T"].tobytes() == got["T"].tobytes() and again["iterations"] == got["iterations"]  # bit-reproducible
    print("largest pose difference, fit_eps %g: %.3e m, %.3e rad" % (fit_eps, worst[0], worst[1]))


# ------------------------------------------------------------------ 4. match()'s scales
@pytest.mark.parametrize("res,steps", [(0.1, 0), (0.1, 2)])
def test_match_scales_against_the_reference(wm, oracle, testscan, res, steps):
    P = synth.make_T((0.2, 0.0, 0.0), (0.0, 0.0, 0.0))
    ref = testscan
    tgt = synth.transform_points(testscan, P)
    T_want, runs = PR.match(oracle, ref, tgt, res=res, multiscale_steps=steps, **YAML)
    assert T_want is not None
    c = wm.Context(0)
    try:
        got = c.icp_match(ref, tgt, res=res, multiscale_steps=steps, mode=wm.WM_ICP_PLANE, **YAML)
    finally:
        c.close()
    print("res %g steps %d: reference iterations per scale %s; device's last %d" % (res, steps, [r["iterations"] for r in runs], got["iterations"]))
    assert got["rc"] == 0
    assert got["iterations"] == runs[-1]["iterations"] and got["state"] == PR.STATE_NAMES[runs[-1]["state"]]
    assert got["n_corr"] == runs[-1]["n_corr"]  # (the last scale's filtered clouds and pose are the reference's)
    dt, ang = pose_error(got["T"], T_want)
    print("    pose vs reference: %.3e m, %.3e rad" % (dt, ang))
    assert dt <= TOL_T and ang <= TOL_R
    assert np.linalg.norm(got["T"] - P) < 0.1


# ------------------------------------------------------------------ 5. degenerate geometry, cached normals
def test_one_plane_ends_degenerate_and_a_new_target_gets_new_normals(wm, ctx):
    rng = np.random.default_rng(3)
    n = 20000
    plane = np.zeros((n, 3), np.float32)
    plane[:, :2] = rng.uniform(-20, 20, (n, 2)).astype(np.float32)
    src = plane[: n // 2] + np.float32([0.05, -0.03, 0.0])
    ctx.set_source(src)
    ctx.set_target(plane)
    L = wm.lib()
    p = wm.icp_params(mode=wm.WM_ICP_PLANE, carry_state=0, **YAML)
    T = np.full((4, 4), 7.25, np.float64)
    s = wm.IcpStats()
    rc = L.wm_icp_align(ctx._h, ctypes.byref(p), T.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(s))
    assert rc == wm.WM_NOT_CONVERGED and s.state == wm.WM_CONV_DEGENERATE and not s.converged and s.iterations == 0
    assert (T == 7.25).all()  # untouched
    assert s.n_corr == n // 2
    # a new target of the SAME size: its normals must be its own
    ref, tgt, _ = synth.pair(n, mode="resample")
    ctx.set_source(ref)
    ctx.set_target(tgt)
    got = ctx.icp_align(mode=wm.WM_ICP_PLANE, carry_state=0, **YAML)
    fresh = wm.Context(0)
    try:
        fresh.set_source(ref)
        fresh.set_target(tgt)
        want = fresh.icp_align(mode=wm.WM_ICP_PLANE, carry_state=0, **YAML)
    finally:
        fresh.close()
    assert got["rc"] == 0 and want["rc"] == 0
    assert got["T"].tobytes() == want["T"].tobytes() and got["iterations"] == want["iterations"]


# ------------------------------------------------------------------ 6. the estimators after a plane align
def test_info_after_a_plane_align(wm, ctx, oracle):
    from test_info_poses_gpu import _check_lum, _check_lumold
    ref, tgt, _ = synth.pair(20000, mode="resample")
    ctx.set_source(ref)
    ctx.set_target(tgt)
    r = ctx.icp_align(mode=wm.WM_ICP_PLANE, carry_state=0, **YAML)
    assert r["rc"] == 0
    idx, _ = ctx.correspondences()
    ok = idx >= 0
    assert ok.sum() == r["n_corr"]
    _check_lum(wm, ctx, oracle, ref, tgt, r["T"], ok, idx)
    _check_lumold(wm, ctx, oracle, ref, tgt, r["T"], 3.0)


# ------------------------------------------------------------------ 7. batch route, sharded refusal
def test_batch_match_takes_the_mode_and_the_sharded_calls_refuse_it(wm, ctx, oracle, testscan):
    pairs = []
    for seed, n in ((3, 1500), (4, 3000)):  # (the smaller one takes the all-pairs search, the others the grid)
        r, t, _ = synth.pair(n, seed=seed, mode="resample")
        pairs.append((r, t))
    r, t, _ = PR.split_pair(oracle, testscan, (0.2, 0.0, 0.0))
    pairs.append((r, t))
    for res, steps in ((-1.0, 0), (0.2, 1)):
        got = ctx.icp_batch_match(pairs, with_info=True, res=res, multiscale_steps=steps, mode=wm.WM_ICP_PLANE, **YAML)
        for (r, t), g in zip(pairs, got):
            one = wm.Context(0)
            try:
                want = one.icp_match(r, t, res=res, multiscale_steps=steps, mode=wm.WM_ICP_PLANE, **YAML)
                rc, info, _ = one.icp_info(wm.WM_INFO_LUMOLD, max_corr=3.0)
            finally:
                one.close()
            assert g["rc"] == want["rc"] == 0
            assert g["T"].tobytes() == want["T"].tobytes()
            assert g["iterations"] == want["iterations"] and g["state"] == want["state"]
            assert rc == 0 and np.array_equal(g["info"], info)
    L = wm.lib()
    p = wm.icp_params(mode=wm.WM_ICP_PLANE, **YAML)
    r, t = pairs[0]
    T = np.zeros((4, 4))
    dp = ctypes.POINTER(ctypes.c_double)
    assert L.wm_icp_align_sharded(ctx._h, None, ctypes.c_void_p(r.ctypes.data), len(r), ctypes.c_void_p(t.ctypes.data), len(t), 12,
                                  wm.WM_MEM_HOST, ctypes.byref(p), T.ctypes.data_as(dp), None) == wm.WM_ERR_ARG
    assert L.wm_icp_shard_begin(ctx._h, ctypes.byref(p), 0.0, 1.0, 0) == wm.WM_ERR_ARG


# ------------------------------------------------------------------ 8. the mode leaves nothing behind
def test_svd_and_gn6_are_the_same_bytes_before_and_after_a_plane_align(wm, ctx):
    ref, tgt, _ = synth.pair(20000, mode="resample", pattern="rings")
    ctx.set_source(ref)
    ctx.set_target(tgt)

    def both():
        out = []
        for mode in (wm.WM_ICP_SVD, wm.WM_ICP_GN6):
            r = ctx.icp_align(mode=mode, carry_state=0, **YAML)
            assert r["rc"] == 0
            idx, d2 = ctx.correspondences()
            out.append((r["T"].tobytes(), r["iterations"], r["state"], r["mse"], r["n_corr"], idx.tobytes(), d2.tobytes(),
                        ctx.icp_stats_for(r["T"], mode).tobytes()))
        return out

    before = both()
    r = ctx.icp_align(mode=wm.WM_ICP_PLANE, carry_state=0, **YAML)
    assert r["rc"] == 0
    assert both() == before
