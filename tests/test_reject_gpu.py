"""Correspondence rejection on the device (wm_icp_params.reject: k_reject_hist, the filtered k_icp_stats / k_plane_stats,
k_reject_mark -- libwave_amd/csrc/wm_reject.hip) against the numpy restatement tests/reject_reference.py: the select bit
for bit, one rejection step, whole registrations, what the feature is for, match()'s scales, the context's
correspondences and the estimators after a rejecting align, the routes, and that rejection leaves nothing behind.

Bounds: the select, the threshold, the counts and the kept mask are EQUAL to the restatement's (integers and bit
patterns); the sums over the kept pairs are within 1e-12 of the largest entry of an extended-precision numpy sum (float64
terms, a fixed summation order: the plane test's bar); helpers.TOL_T / TOL_R for poses.  The largest differences belong
in DESIGN.md section 4.9; every test prints its own."""
import ctypes

import numpy as np
import pytest

import plane_reference as PR
import reject_reference as RR
from helpers import TOL_R, TOL_T, pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu

YAML = dict(max_corr=3.0, max_iter=100, t_eps=1e-8, fit_eps=1e-2)  # tests/golden/config/icp.yaml
POSES = [np.eye(4), synth.make_T((0.15, -0.1, 0.05), (0.01, -0.02, 0.015)), synth.make_T((-0.3, 0.2, -0.1), (-0.02, 0.01, 0.04))]
RULES = {"trimmed": dict(reject=RR.TRIMMED, ratio=0.5), "median": dict(reject=RR.MEDIAN, factor=1.0)}


def _dev_kw(kw):
    """the restatement's keywords -> wm_icp_params fields"""
    names = dict(reject="reject", ratio="reject_ratio", factor="reject_factor", min_corr="reject_min_corr")
    return {names[k]: v for k, v in kw.items()}


# ------------------------------------------------------------------ 1. the select, bit for bit
@pytest.mark.parametrize("n", RR.SELECT_LENGTHS)
def test_rank_select_bit_for_bit(wm, ctx, n):
    for name, vals in RR.crafted(n).items():
        b = vals.view(np.uint32)
        for rank in RR.select_ranks(n):
            want = np.partition(b, rank)[rank]
            got = ctx.debug_rank_select(vals, rank)
            assert got.reshape(1).view(np.uint32)[0] == want, (name, n, rank, got, want)


# ------------------------------------------------------------------ 2. one rejection step
def _ld_sums(mode, pf, q, nrm, d2):
    """the public 32-slot block of a mode over the given pairs, summed in extended precision (slots 0 ... 28)"""
    ld = np.longdouble
    p, q = pf.astype(ld), q.astype(ld)
    st = np.zeros(29, ld)
    st[0] = len(p)
    sd2 = d2.astype(ld).sum()
    if mode == RR.SVD:
        st[1:4] = p.sum(0)
        st[4:7] = q.sum(0)
        st[7:16] = np.array([[(q[:, a] * p[:, b]).sum() for b in range(3)] for a in range(3)]).reshape(-1)
        st[16] = sd2
        return st
    st[1] = sd2
    if mode == RR.GN6:
        r = p - q
        H = np.zeros((6, 6), ld)
        sp = p.sum(0)
        H[0, 0] = H[1, 1] = H[2, 2] = len(p)
        H[0, 4], H[0, 5], H[1, 3], H[1, 5], H[2, 3], H[2, 4] = sp[2], -sp[1], -sp[2], sp[0], sp[1], -sp[0]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        H[3, 3], H[3, 4], H[3, 5] = (y * y + z * z).sum(), (-x * y).sum(), (-x * z).sum()
        H[4, 4], H[4, 5], H[5, 5] = (x * x + z * z).sum(), (-y * z).sum(), (x * x + y * y).sum()
        g = np.concatenate([r.sum(0), np.cross(p, r).sum(0)])
    else:
        n = nrm.astype(ld)
        has = (n != 0).any(1)
        p, q, n = p[has], q[has], n[has]
        J = np.concatenate([n, np.cross(p, n)], axis=1)
        r = (n * (p - q)).sum(1)
        H = np.array([[(J[:, a] * J[:, b]).sum() for b in range(6)] for a in range(6)])
        g = np.array([(J[:, a] * r).sum() for a in range(6)])
    st[2:23] = H[np.triu_indices(6)]
    st[23:29] = g
    return st


def _step_params(n_matched):
    out = [dict(reject=RR.TRIMMED, ratio=r, min_corr=m) for r in (1.0, 0.5, 0.3, 1e-9) for m in (0, 5, n_matched + 1)]
    out += [dict(reject=RR.MEDIAN, factor=f) for f in (0.0, 1.0, 4.0, 1e30)]
    return out


def _check_steps(wm, ctx, src, tgt, T, what, nn=None):
    """wm_nn_search under T, then every parameter set of the issue: the device's step against the restatement's on the
    device's own correspondences; sums in all three modes; a second call; ratio 1.0 against wm_icp_stats_for"""
    ctx.set_source(src)
    ctx.set_target(tgt)
    nrm = ctx.estimate_normals(1, 20)
    ctx.nn_search(T, max_corr=3.0, nn_method=wm.WM_NN_GRID if nn is None else nn)
    idx, d2 = ctx.correspondences()
    ok = idx >= 0
    pf = PR.transform_f32(src, T)
    n_fin = int(np.isfinite(src).all(1).sum())
    worst = 0.0
    for kw in _step_params(int(ok.sum())):
        want = RR.reject_step(d2[ok], **kw)
        kept = np.zeros(len(src), bool)
        kept[np.nonzero(ok)[0][want["kept"]]] = True
        for mode in (wm.WM_ICP_SVD, wm.WM_ICP_GN6, wm.WM_ICP_PLANE):
            got = ctx.icp_reject(T, mode=mode, **kw)
            assert got["n_matched"] == want["n_matched"] == ok.sum(), (what, kw, got["n_matched"], want["n_matched"])
            assert got["n_kept"] == want["n_kept"], (what, kw, got["n_kept"], want["n_kept"])
            assert got["threshold_d2"].reshape(1).view(np.uint32)[0] == want["threshold"].reshape(1).view(np.uint32)[0], (what, kw)
            assert got["all_kept"] == want["all_kept"], (what, kw)
            assert np.array_equal(got["kept"], kept), (what, kw)
            st = got["stats"]
            assert st[0] == want["n_kept"] and st[31] == n_fin
            ref = _ld_sums(mode, pf[kept], tgt[idx[kept]], nrm[idx[kept], :3], d2[kept])
            scale = float(np.abs(ref).max())
            err = float(np.abs(st[:29].astype(np.longdouble) - ref).max()) / scale if scale > 0 else float(np.abs(st[:29]).max())
            worst = max(worst, err)
            assert err <= 1e-12, (what, kw, mode, err)
            again = ctx.icp_reject(T, mode=mode, **kw)
            assert again["stats"].tobytes() == st.tobytes() and np.array_equal(again["kept"], got["kept"])
            assert (again["n_matched"], again["n_kept"], again["threshold_d2"].tobytes()) == (got["n_matched"], got["n_kept"], got["threshold_d2"].tobytes())
            if kw.get("ratio") == 1.0:
                assert st.tobytes() == ctx.icp_stats_for(T, mode).tobytes(), (what, kw, mode)
    # the step leaves the context's correspondences as they are
    idx2, d22 = ctx.correspondences()
    assert np.array_equal(idx2, idx) and np.array_equal(d22, d2)
    print("%s: %d matched of %d, largest sum error %.3e of the largest entry" % (what, ok.sum(), len(src), worst))


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_one_step_on_the_resample_pair(wm, ctx, pose):
    ref, tgt, _ = synth.pair(20000, mode="resample")
    _check_steps(wm, ctx, ref, tgt, POSES[pose], "resample, pose %d" % pose)


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_one_step_with_non_finite_and_unmatched_queries(wm, ctx, pose):
    ref, tgt, _ = synth.pair(20000, mode="resample")
    ref = ref.copy()
    ref[5] = np.nan
    ref[77, 1] = np.inf
    ref[1000:1003, 2] = -np.inf
    ref[0::4] += np.float32([0.0, 0.0, 500.0])  # a quarter of the source beyond max_corr: counts for nothing
    _check_steps(wm, ctx, ref, tgt, POSES[pose], "non-finite + unmatched, pose %d" % pose)


def test_one_step_where_every_distance_ties(wm, ctx):
    ref, tgt, T = synth.pair(20000, mode="copy")
    _check_steps(wm, ctx, ref, tgt, T, "copy at its true pose")
    g = np.arange(20, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    shifted = lattice + np.float32([0.5, 0.0, 0.0])
    ctx.set_source(shifted)
    ctx.set_target(lattice)
    _, d2 = ctx.nn_search(np.eye(4), max_corr=3.0)
    assert (d2 == np.float32(0.25)).all()  # all equal, not zero
    _check_steps(wm, ctx, shifted, lattice, np.eye(4), "lattice shifted by half a cell")


@pytest.mark.parametrize("m", [0, 1, 2, 3, 65])
def test_one_step_with_few_matched_points(wm, ctx, m):
    ref, tgt, _ = synth.pair(4000, seed=9, mode="resample")
    far = ref[:3] + np.float32([0.0, 0.0, 900.0])
    src = np.concatenate([ref[100:100 + m], far]).astype(np.float32)
    _check_steps(wm, ctx, src, tgt, POSES[1], "%d matched points" % m, nn=wm.WM_NN_BRUTE if m == 2 else None)


# ------------------------------------------------------------------ 3. whole registrations against the restatement
_PAIRS = {}
_WANT = {}


def _pair(oracle, testscan, name):
    if name not in _PAIRS:
        if name == "partial":
            _PAIRS[name] = RR.partial_pair()
        elif name in ("uniform", "rings"):
            _PAIRS[name] = synth.pair(20000, mode="resample", pattern=name)
        else:
            tt, yaw, pitch = PR.SPLIT_PERTURBATIONS[int(name[-1])]
            _PAIRS[name] = PR.split_pair(oracle, testscan, tt, yaw, pitch)
    return _PAIRS[name]


_NORMALS = {}


def _normals(ctx, name, tgt):
    """The plane registrations' restatement takes the DEVICE's normals of the target (checked on their own against
    PR.normals, tests/test_icp_plane_gpu.py: 1e-6 rad).  With the restatement's float64 normals against the device's
    stored float32 ones the poses of a plane registration agree to 1e-8 m (measured: 9.2e-8 m at the most, against 1.5e-13
    for SVD / GN6); that moves the mean d2 of the kept pairs by 3e-7 of itself, which is 0.6 of what the relative-MSE rule
    compares with at fit_eps = 1e-6 -- measured: the partial pair under the median rule stopped at iteration 18
    (REL_MSE) on the device and 19 (TRANSFORM) in the restatement, whose margin there was 0.013.  With the same
    normals on both sides what is compared is the rejection and the loop."""
    if name not in _NORMALS:
        ctx.set_target(tgt)
        ctx.set_source(tgt[:64])
        _NORMALS[name] = ctx.estimate_normals(1, PR.DEFAULT_K)[:, :3].astype(np.float64)
    return _NORMALS[name]


def _reference(ctx, oracle, testscan, name, rule, mode, fit_eps):
    key = (name, rule, mode, fit_eps)
    if key not in _WANT:
        ref, tgt, _ = _pair(oracle, testscan, name)
        nrm = _normals(ctx, name, tgt) if mode == RR.PLANE else None
        _WANT[key] = RR.align(oracle, ref, tgt, mode=mode, tgt_normals=nrm, **RULES[rule], **dict(YAML, fit_eps=fit_eps))
    return _WANT[key]


def _registration(wm, ctx, oracle, testscan, name, rule, mode, fit_eps):
    ref, tgt, _ = _pair(oracle, testscan, name)
    want = _reference(ctx, oracle, testscan, name, rule, mode, fit_eps)
    assert want["margin"] > 1e-6, (name, rule, mode, want["margin"])  # (else: another seed)
    ctx.set_source(ref)
    ctx.set_target(tgt)
    kw = dict(mode=mode, carry_state=0, **_dev_kw(RULES[rule]), **dict(YAML, fit_eps=fit_eps))
    got = ctx.icp_align(**kw)
    again = ctx.icp_align(**kw)
    print("%s %s mode %d fit_eps %g: %d iterations (%s), reference %d (%s); kept %d of %d" %
          (name, rule, mode, fit_eps, got["iterations"], got["state"], want["iterations"], PR.STATE_NAMES[want["state"]],
           got["n_corr"], got["n_matched"]))
    assert got["rc"] == 0 and want["converged"], (name, rule, mode, got)
    assert got["iterations"] == want["iterations"], (name, rule, mode, got["iterations"], want["iterations"])
    assert got["state"] == PR.STATE_NAMES[want["state"]], (name, rule, mode, got["state"])
    assert got["n_corr"] == want["n_corr"] and got["n_matched"] == want["n_matched"], (name, rule, mode)
    # (the threshold's bits are compared where the pose is the same on both sides: one rejection step, above)
    dt, ang = pose_error(got["T"], want["T"])
    print("    pose vs reference: %.3e m, %.3e rad" % (dt, ang))
    assert dt <= TOL_T and ang <= TOL_R, (name, rule, mode, dt, ang)
    assert again["T"].tobytes() == got["T"].tobytes()  # bit-reproducible
    assert (again["iterations"], again["state"], again["n_corr"], again["n_matched"], again["mse"], again["reject_d2"]) == \
           (got["iterations"], got["state"], got["n_corr"], got["n_matched"], got["mse"], got["reject_d2"])
    return dt, ang


@pytest.mark.parametrize("fit_eps", [1e-2, 1e-6])
@pytest.mark.parametrize("name", ["partial", "uniform", "rings", "split0", "split1", "split2"])
def test_registrations_against_the_reference(wm, ctx, oracle, testscan, name, fit_eps):
    worst = (0.0, 0.0)
    for rule in RULES:
        for mode in (RR.SVD, RR.PLANE):
            dt, ang = _registration(wm, ctx, oracle, testscan, name, rule, mode, fit_eps)
            worst = (max(worst[0], dt), max(worst[1], ang))
    if name == "uniform":
        dt, ang = _registration(wm, ctx, oracle, testscan, name, "trimmed", RR.GN6, fit_eps)
        worst = (max(worst[0], dt), max(worst[1], ang))
    print("largest pose difference, %s, fit_eps %g: %.3e m, %.3e rad" % (name, fit_eps, worst[0], worst[1]))


# ------------------------------------------------------------------ 4. what it is for
def test_partial_overlap_needs_rejection_on_the_device(wm, ctx):
    ref, tgt, T_gt = RR.partial_pair()
    ctx.set_source(ref)
    ctx.set_target(tgt)
    kw = dict(YAML, fit_eps=1e-6, carry_state=0)
    plain = ctx.icp_align(**kw)
    far = plain["rc"] != 0 or pose_error(plain["T"], T_gt)[0] > 1.0
    print("plain: rc %d, %d iterations (%s)%s" % (plain["rc"], plain["iterations"], plain["state"],
                                                  "" if plain["T"] is None else ", %.3f m from the true pose" % pose_error(plain["T"], T_gt)[0]))
    assert far
    assert plain["n_matched"] == plain["n_corr"] and plain["reject_d2"] == 0.0
    trimmed = ctx.icp_align(reject=wm.WM_REJECT_TRIMMED, reject_ratio=0.5, **kw)
    assert trimmed["rc"] == 0
    dt, ang = pose_error(trimmed["T"], T_gt)
    print("trimmed 0.5: %d iterations (%s), %.4f m, %.3e rad; kept %d of %d" %
          (trimmed["iterations"], trimmed["state"], dt, ang, trimmed["n_corr"], trimmed["n_matched"]))
    assert dt <= 0.05 and ang <= 0.01
    assert trimmed["n_corr"] < trimmed["n_matched"]


# ------------------------------------------------------------------ 5. match()'s scales
@pytest.mark.parametrize("res,steps", [(0.1, 0), (0.1, 2)])
def test_match_scales_against_the_reference(wm, oracle, testscan, res, steps):
    P = synth.make_T((0.2, 0.0, 0.0), (0.0, 0.0, 0.0))
    ref = testscan
    tgt = synth.transform_points(testscan, P)
    T_want, runs = RR.match(oracle, ref, tgt, res=res, multiscale_steps=steps, reject=RR.TRIMMED, ratio=0.7, **YAML)
    assert T_want is not None and all(r["margin"] > 1e-6 for r in runs)
    c = wm.Context(0)
    try:
        got = c.icp_match(ref, tgt, res=res, multiscale_steps=steps, reject=wm.WM_REJECT_TRIMMED, reject_ratio=0.7, **YAML)
    finally:
        c.close()
    print("res %g steps %d: reference iterations per scale %s; device's last %d" % (res, steps, [r["iterations"] for r in runs], got["iterations"]))
    assert got["rc"] == 0
    assert got["iterations"] == runs[-1]["iterations"] and got["state"] == PR.STATE_NAMES[runs[-1]["state"]]
    assert got["n_corr"] == runs[-1]["n_corr"] and got["n_matched"] == runs[-1]["n_matched"]
    dt, ang = pose_error(got["T"], T_want)
    print("    pose vs reference: %.3e m, %.3e rad" % (dt, ang))
    assert dt <= TOL_T and ang <= TOL_R
    assert np.linalg.norm(got["T"] - P) < 0.1


# ------------------------------------------------------------------ 6. after the align
@pytest.mark.parametrize("rule", ["trimmed", "median"])
def test_correspondences_and_estimators_after_a_rejecting_align(wm, ctx, oracle, rule):
    from test_info_poses_gpu import _check_censi, _check_lum, _check_lumold
    ref, tgt, _ = synth.pair(20000, mode="resample")
    want = RR.align(oracle, ref, tgt, **RULES[rule], **YAML)
    ctx.set_source(ref)
    ctx.set_target(tgt)
    r = ctx.icp_align(carry_state=0, **_dev_kw(RULES[rule]), **YAML)
    assert r["rc"] == 0 and r["iterations"] == want["iterations"]
    idx, d2 = ctx.correspondences()
    ok = idx >= 0
    assert ok.sum() == r["n_corr"] == want["n_corr"]
    assert np.array_equal(np.nonzero(ok)[0], np.sort(want["kept_src"]))
    order = np.argsort(want["kept_src"])
    assert np.array_equal(idx[ok], want["kept_tgt"][order])
    # a rejected pair keeps its d2: every matched query's distance is there, the rejected ones' above the threshold
    thr = np.float32(r["reject_d2"])
    assert (d2[ok] <= thr).all()
    assert ((idx == -1) & (d2 > thr) & np.isfinite(d2)).sum() >= r["n_matched"] - r["n_corr"] > 0
    _check_lum(wm, ctx, oracle, ref, tgt, r["T"], ok, idx)
    _check_censi(wm, ctx, oracle, ref[ok], tgt[idx[ok]], r["T"])
    _check_lumold(wm, ctx, oracle, ref, tgt, r["T"], 3.0)


# ------------------------------------------------------------------ 7. routes
def test_batch_match_takes_rejection_and_the_sharded_calls_refuse_it(wm, ctx, oracle, testscan):
    pairs = []
    for seed, n in ((3, 1500), (4, 3000)):  # (the smaller one takes the all-pairs search, the other the grid)
        r, t, _ = synth.pair(n, seed=seed, mode="resample")
        pairs.append((r, t))
    r, t, _ = PR.split_pair(oracle, testscan, (0.2, 0.0, 0.0))
    pairs.append((r, t))
    rej = dict(reject=wm.WM_REJECT_TRIMMED, reject_ratio=0.6)
    for res, steps in ((-1.0, 0), (0.2, 1)):
        got = ctx.icp_batch_match(pairs, with_info=True, res=res, multiscale_steps=steps, **rej, **YAML)
        for (r, t), g in zip(pairs, got):
            one = wm.Context(0)
            try:
                want = one.icp_match(r, t, res=res, multiscale_steps=steps, **rej, **YAML)
                rc, info, _ = one.icp_info(wm.WM_INFO_LUMOLD, max_corr=3.0)
            finally:
                one.close()
            assert g["rc"] == want["rc"] == 0
            assert g["T"].tobytes() == want["T"].tobytes()
            assert (g["iterations"], g["state"], g["n_corr"], g["n_matched"]) == (want["iterations"], want["state"], want["n_corr"], want["n_matched"])
            assert g["n_corr"] < g["n_matched"]
            assert rc == 0 and np.array_equal(g["info"], info)
    L = wm.lib()
    p = wm.icp_params(**rej, **YAML)
    r, t = pairs[0]
    T = np.zeros((4, 4))
    dp = ctypes.POINTER(ctypes.c_double)
    assert L.wm_icp_align_sharded(ctx._h, None, ctypes.c_void_p(r.ctypes.data), len(r), ctypes.c_void_p(t.ctypes.data), len(t), 12,
                                  wm.WM_MEM_HOST, ctypes.byref(p), T.ctypes.data_as(dp), None) == wm.WM_ERR_ARG
    assert L.wm_icp_shard_begin(ctx._h, ctypes.byref(p), 0.0, 1.0, 0) == wm.WM_ERR_ARG
    m = wm.Multi([0])
    try:
        with pytest.raises(wm.WmError, match="-1|argument"):
            m.icp_match(r, t, params=p)
        assert m.icp_match(r, t, **YAML)["rc"] == 0  # (the group itself works)
    finally:
        m.close()


def test_invalid_parameters_and_a_rule_that_rejects_everything(wm, ctx):
    ref, tgt, _ = synth.pair(20000, mode="resample")
    ctx.set_source(ref)
    ctx.set_target(tgt)
    L = wm.lib()
    T = np.full((4, 4), 7.25)
    dp = ctypes.POINTER(ctypes.c_double)
    for bad in (dict(reject=3), dict(reject=-1), dict(reject=1, reject_ratio=-0.1), dict(reject=1, reject_ratio=1.5),
                dict(reject=1, reject_ratio=float("nan")), dict(reject=2, reject_factor=-1.0), dict(reject=2, reject_factor=float("inf")),
                dict(reject=1, reject_min_corr=-1)):
        p = wm.icp_params(**bad, **YAML)
        assert L.wm_icp_align(ctx._h, ctypes.byref(p), T.ctypes.data_as(dp), None) == wm.WM_ERR_ARG, bad
    # k == 0: everything is rejected -> fewer than 3 pairs -> NO_CORRESPONDENCES, T untouched, no pair left
    p = wm.icp_params(reject=wm.WM_REJECT_TRIMMED, reject_ratio=1e-9, carry_state=0, **YAML)
    s = wm.IcpStats()
    rc = L.wm_icp_align(ctx._h, ctypes.byref(p), T.ctypes.data_as(dp), ctypes.byref(s))
    assert rc == wm.WM_TOO_FEW and wm.CONV_NAMES[s.state] == "NO_CORRESPONDENCES" and s.iterations == 0
    assert (T == 7.25).all()
    assert s.n_corr == 0 and s.n_matched > 0 and s.reject_d2 == -1.0
    idx, d2 = ctx.correspondences()
    assert (idx == -1).all() and (d2 > 0).sum() > 0
    # min_corr beyond the matched count: nothing is rejected -- the bytes of an align without rejection
    plain = ctx.icp_align(carry_state=0, **YAML)
    kept = ctx.icp_align(carry_state=0, reject=wm.WM_REJECT_TRIMMED, reject_ratio=0.2, reject_min_corr=len(ref) + 1, **YAML)
    assert kept["rc"] == plain["rc"] == 0 and kept["iterations"] == plain["iterations"] and kept["n_corr"] == plain["n_corr"] == kept["n_matched"]
    dt, ang = pose_error(kept["T"], plain["T"])
    assert dt <= 1e-9 and ang <= 1e-9  # (the same pairs; sums by rows of partial sums here, by bins there)
    assert kept["reject_d2"] == RR.FLT_MAX


# ------------------------------------------------------------------ 8. nothing left behind
def test_aligns_without_rejection_are_the_same_bytes_before_and_after(wm, ctx):
    ref, tgt, _ = synth.pair(20000, mode="resample", pattern="rings")

    def all_three(c):
        out = []
        for mode in (wm.WM_ICP_SVD, wm.WM_ICP_GN6, wm.WM_ICP_PLANE):
            r = c.icp_align(mode=mode, carry_state=0, **YAML)
            assert r["rc"] == 0 and r["n_matched"] == r["n_corr"] and r["reject_d2"] == 0.0
            idx, d2 = c.correspondences()
            out.append((r["T"].tobytes(), r["iterations"], r["state"], r["mse"], r["n_corr"], idx.tobytes(), d2.tobytes(),
                        c.icp_stats_for(r["T"], mode).tobytes()))
        return out

    ctx.set_source(ref)
    ctx.set_target(tgt)
    before = all_three(ctx)
    for mode in (wm.WM_ICP_SVD, wm.WM_ICP_PLANE):
        for rule in RULES.values():
            r = ctx.icp_align(mode=mode, carry_state=0, **_dev_kw(rule), **YAML)
            assert r["rc"] == 0 and r["n_corr"] < r["n_matched"]
    assert all_three(ctx) == before
    fresh = wm.Context(0)
    try:
        fresh.set_source(ref)
        fresh.set_target(tgt)
        assert all_three(fresh) == before
    finally:
        fresh.close()
