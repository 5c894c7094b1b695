"""tests/icp_reference.py held on the CPU: its pairs to the oracle's kd-tree, its steps to the oracle's (oracle/icp.c,
oracle/linalg.c), its case inventory, the REF_FORMS table -- and the library's HOST build of the solve (wm_math.hpp through
wm.umeyama_from_stats / wm.gn6_from_stats / wm.HostIcp) to the reference on correctly rounded sums.  No device.

What this file found, on the host build, before any kernel was run:
  * gn6_from_stats on a singular J^T J (collinear or coincident pairs) did not merely "fall back": chol_solve replaced a
    non-positive pivot by 1 and reported it, icp_apply_stats ignored the report, and where the pivot came out POSITIVE at
    rounding level (1e-15 of its diagonal entry) nothing was reported at all.  Measured on correctly rounded sums: the
    sum of squared residuals of `point` went from 0.15 to 1.1e8, of `collinear3` from 0.53 to 2.8e13, of `line_far` from
    5.2 to 5.6e4, of `line_diag` from 1.9 to 7.3.  Fixed: a pivot at or below 1e-12 of its own diagonal entry is
    singular (kGnPivotTol), the iteration ends WM_CONV_DEGENERATE with the pose untouched, on every path; the oracle
    states the same rule.  Regular cases keep their bits (the branch is not taken: their smallest pivot is 1.1e-8 of its
    entry, on utm_plane; the largest pivot of a singular case 6.7e-15 -- test_gn6_pivots_leave_a_gap prints both).
  * the 32 random lines below were benign under the old rule (the residual fell from 0.36 to below 1e-5 on each), by
    luck: which of them "failed" went by the sign of a pivot at rounding level.  With the rule 31 are reported and
    not stepped; the one that passes is the least singular (pivot 6e-11) and reaches the reference's residual.
  * `mirror` (the scene against its target mirrored in z) does NOT reach the det(U) det(V) < 0 branch: nearest-neighbour
    pairing matches a point with whatever of the mirrored cloud is near it, and sigma's determinant stays positive
    (+2.6e5).  `mirror_thin` (a 1 cm slab with points 36 cm apart) pairs every point with its own image and does.
  * GN6 linearises the rotation about the ORIGIN: from the identity on `utm` (55 km out, a motion of 3.7e-3 rad) the exact
    step leaves 0.5 |dw|^2 |p| = 0.38 m per point, the sum of squared residuals goes from 17.7 to 301 -- library and
    reference agree on that step to 4e-10 m.  The four properties are therefore asserted at each case's pairing pose
    (what REF_FORMS is defined on); test_gn6_overshoots_far_from_the_origin pins the overshoot as the method's own."""
import numpy as np
import pytest

import gicp_reference as GR
import icp_reference as IR
from helpers import TOL_T, pose_error

I4 = np.eye(4, dtype=np.float32)
LD = np.longdouble
WITH_STEP = [n for n in IR.NAMES if n not in ("no_pair", "one_pair")]  # at least three pairs under both poses


def _pq(c, Tf):
    idx, d2 = c.pairs_at(Tf)
    si, p, q = IR.matched(c.src, c.tgt, Tf, idx)
    return si, p, q, d2[si]


def _lib_step(wm, p, q, d2, mode):
    st, _ = IR.sums(p, q, d2, mode)
    rc, T = (wm.umeyama_from_stats if mode == IR.SVD else wm.gn6_from_stats)(st)
    return rc, T, st


# ------------------------------------------------------------------------------------------------- the pairs
@pytest.mark.parametrize("name", IR.NAMES)
def test_pairs_equal_the_oracles_kdtree_and_gate(oracle, name):
    c = IR.case(name)
    src, tgt = c.finite()
    fs, ft = np.nonzero(np.isfinite(c.src).all(1))[0], np.nonzero(np.isfinite(c.tgt).all(1))[0]
    tree = oracle.KdTree(tgt)
    for Tf in (c.T0f, I4):
        oi, od = tree.nn(oracle.transform_cloud_f(src, Tf))
        keep = od.astype(np.float64) <= c.max_corr * c.max_corr  # (oracle/icp.c rejects d2 > max_d2)
        want = np.full(len(c.src), -1, np.int32)
        want[fs] = np.where(keep, ft[oi], -1)
        idx, d2 = c.pairs_at(Tf)
        assert np.array_equal(idx, want)
        assert np.array_equal(d2[fs][keep], od[keep]) and not d2[idx < 0].any()


def test_case_inventory():
    C = IR.cases()
    assert all(len(c.src) <= 3375 and len(c.tgt) <= 3375 for c in C.values())
    for k in IR.PAIRS_K:
        c = C["pairs%d" % k]
        assert len(c.src) == 3000 and (~np.isfinite(c.src).all(1)).sum() == 4
        for idx, _ in (c.pairs(), c.pairs_identity()):
            rows = np.nonzero(idx >= 0)[0]
            assert len(rows) == k
            # spread through the order: in every twelfth of the source (a workgroup of kBlock rows), holes inside the stretch
            assert len(set(rows // 256)) == 12 and rows[0] < 64 and rows[-1] >= 2900
            holes = np.nonzero(~np.isfinite(c.src).all(1))[0]
            assert rows[0] < holes.min() and holes.max() < rows[-1]
    for idx, _ in (C["collinear3"].pairs(), C["collinear3"].pairs_identity()):
        assert (idx >= 0).sum() == 3
    si, p, _, _ = _pq(C["collinear3"], C["collinear3"].T0f)
    assert np.linalg.matrix_rank(p.astype(np.float64) - p.astype(np.float64).mean(0), tol=1e-5) == 1
    # the pair exactly on the gate is kept: one more than under GICP's strict gate, at the pose the gate was taken under
    for name, Tf in (("half", C["half"].T0f), ("half_start", I4)):
        c = C[name]
        idx, d2 = c.pairs_at(Tf)
        strict, _ = GR.pairs(c.src, c.tgt, Tf, c.max_corr)
        on_gate = (idx >= 0) & (d2.astype(np.float64) == c.max_corr * c.max_corr)
        assert on_gate.sum() == 1 and (idx >= 0).sum() == (strict >= 0).sum() + 1
        assert np.array_equal(idx[~on_gate], strict[~on_gate])
    for n in (1023, 1024, 1025):
        assert len(C["n%d" % n].src) == n
    # which mirrored case reaches Umeyama's reflection branch (det(U) det(V) < 0 <=> det(sigma) < 0)
    dets = {}
    for name in ("mirror", "mirror_thin"):
        for Tf in (C[name].T0f, I4):
            _, p, q, _ = _pq(C[name], Tf)
            pd, qd = p.astype(np.float64), q.astype(np.float64)
            dets[(name, Tf is I4)] = np.linalg.det((qd - qd.mean(0)).T @ (pd - pd.mean(0)) / len(pd))
    print(dets)
    assert all((d < 0) == (name == "mirror_thin") for (name, _), d in dets.items())
    for name in IR.FREE:
        _, p, _, _ = _pq(C[name], C[name].T0f)
        assert np.linalg.matrix_rank(p.astype(np.float64) - p.astype(np.float64).mean(0), tol=1e-4) <= 1, name


# ------------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("name", [n for n in WITH_STEP if n not in IR.FREE])
def test_steps_match_the_oracles(oracle, name):
    """step(SVD) against oracle.umeyama on the same pairs, step(GN6) against the oracle's one forced GN6 iteration (its
    own search, from the identity): 1e-9 m / 1e-9 rad, the figure of test_capi_cpu.py::test_host_umeyama_matches_oracle"""
    c = IR.case(name)
    for Tf in (c.T0f, I4):
        _, p, q, _ = _pq(c, Tf)
        dt, ang = pose_error(IR.step(p, q, IR.SVD), oracle.umeyama(p, q))
        print(name, "svd", "%.2e m %.2e rad" % (dt, ang))
        assert dt <= 1e-9 and ang <= 1e-9, (name, dt, ang)
    _, p, q, _ = _pq(c, I4)
    for mode_name, mode in IR.MODES:
        one = oracle.icp_align(*c.finite(), max_corr=c.max_corr, force_iterations=1, mode=mode, incremental_float=0)
        assert one["state"] == "FORCED" and one["n_corr"] == len(p)
        dt, ang = pose_error(IR.step(p, q, mode), one["T"])
        print(name, mode_name, "forced iteration: %.2e m %.2e rad" % (dt, ang))
        assert dt <= 1e-9 and ang <= 1e-9, (name, mode_name, dt, ang)


# ------------------------------------------------------------------------- the library's host solve: REF_FORMS
def _forms(wm, name):
    """disp between the library's formula on correctly rounded sums and step(), the larger of the two poses the GPU
    tests pair under (the case's own and the identity); None where the library refuses the system"""
    c = IR.case(name)
    out = []
    for _, mode in IR.MODES:
        worst = 0.0
        for Tf in (c.T0f, I4):
            _, p, q, d2 = _pq(c, Tf)
            rc, T, _ = _lib_step(wm, p, q, d2, mode)
            if rc != wm.WM_OK:
                worst = None
                break
            worst = max(worst, IR.disp(T, IR.step(p, q, mode), IR.compare_points(c, Tf, p)))
        out.append(worst)
    return tuple(out)


def test_ref_forms_table(wm):
    assert sorted(IR.REF_FORMS) == sorted(WITH_STEP)
    bad = []
    for name in WITH_STEP:
        got = _forms(wm, name)
        print('    "%s": (%s),' % (name, ", ".join("None" if g is None else "%.1e" % g for g in got)))
        for g, t in zip(got, IR.REF_FORMS[name]):
            # the table holds the measured value rounded up: not below it, and not a decade above it (below 1e-16 --
            # `point`, where every form gives the same bits -- the table says 1e-16)
            if (g is None) != (t is None) or (g is not None and not (g <= t <= max(10.0 * g, 1e-16))):
                bad.append((name, got, IR.REF_FORMS[name]))
    assert not bad, bad
    # refused: GN6 on exactly the FREE cases
    assert {n for n in WITH_STEP if IR.REF_FORMS[n][1] is None} == IR.FREE
    assert all(IR.REF_FORMS[n][0] is not None for n in WITH_STEP)


def _properties(T, T_ref, p, q, delta):
    """the four properties of a step: finite; orthonormal, det +1 to 1e-12; the sum of squared residuals does not rise;
    it reaches the reference's minimum to within what moving every point by delta can add (IR.ssr_slack)"""
    assert np.isfinite(T).all()
    orth, det = IR.rigid_error(T)
    assert orth <= 1e-12 and det <= 1e-12, (orth, det)
    before, after, ref = IR.ssr(np.eye(4), p, q), IR.ssr(T, p, q), IR.ssr(T_ref, p, q)
    assert after <= before, (before, after)
    assert after <= ref + IR.ssr_slack(delta, T_ref, p, q), (after, ref, delta)
    return before, after, ref


@pytest.mark.parametrize("name", WITH_STEP)
def test_host_step_from_rounded_sums(wm, name):
    c = IR.case(name)
    _, p, q, d2 = _pq(c, c.T0f)
    for (mode_name, mode), form in zip(IR.MODES, IR.REF_FORMS[name]):
        rc, T, st = _lib_step(wm, p, q, d2, mode)
        if mode == IR.GN6 and name in IR.FREE:
            # singular J^T J: reported, whichever way the pivot's sign falls, and never stepped (test_host_icp_*)
            assert rc == wm.WM_NOT_CONVERGED and np.isfinite(T).all(), (name, rc)
            continue
        assert rc == wm.WM_OK
        delta = 100.0 * form + IR.pose_floor(p, q)
        before, after, ref = _properties(T, IR.step(p, q, mode), p, q, delta)
        print("%s %s: residual %.6e -> %.6e (reference %.6e), allowed displacement %.1e m" % (name, mode_name, before, after, ref, delta))


def test_gn6_overshoots_far_from_the_origin(wm):
    """from the identity on `utm` the exact Gauss-Newton step RAISES the residual: the rotation is linearised about the
    origin, 55 km away.  Library and reference take the same step (REF_FORMS); the overshoot is the method's."""
    c = IR.case("utm")
    _, p, q, d2 = _pq(c, I4)
    rc, T, _ = _lib_step(wm, p, q, d2, IR.GN6)
    Tr = IR.step(p, q, IR.GN6)
    before, lib, ref = IR.ssr(np.eye(4), p, q), IR.ssr(T, p, q), IR.ssr(Tr, p, q)
    print("utm gn6 from the identity: %.4e -> library %.4e, reference %.4e; disp %.1e" % (before, lib, ref, IR.disp(T, Tr, p)))
    assert rc == wm.WM_OK and IR.disp(T, Tr, p) <= 100.0 * IR.REF_FORMS["utm"][1]
    assert lib > 10 * before and abs(lib - ref) <= 1e-6 * ref
    # ... and the SVD step does not
    rc, T, _ = _lib_step(wm, p, q, d2, IR.SVD)
    assert IR.ssr(T, p, q) < 1e-3 * before


def _chol_pivots(st):
    """the Cholesky pivots of the public GN6 slots, each relative to its own diagonal entry (numpy, as chol_solve)"""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = st[2:23]
    H = H + np.triu(H, 1).T
    L = np.zeros((6, 6))
    rel = []
    for i in range(6):
        for j in range(i + 1):
            s = H[i, j] - sum(L[i, k] * L[j, k] for k in range(j))
            if i == j:
                rel.append(s / H[i, i] if H[i, i] > 0 else 0.0)
                L[i, i] = np.sqrt(s) if s > 0 else 1.0
            else:
                L[i, j] = s / L[j, j]
    return rel


def test_gn6_pivots_leave_a_gap():
    """kGnPivotTol = 1e-12 sits four decades below the smallest pivot of a regular case and two above the largest of a
    singular one (only the first non-positive or tiny pivot of a singular system means anything)"""
    regular, singular = {}, {}
    for name in WITH_STEP:
        c = IR.case(name)
        for Tf in (c.T0f, I4):
            _, p, q, d2 = _pq(c, Tf)
            rel = _chol_pivots(IR.sums(p, q, d2, IR.GN6)[0])
            if name in IR.FREE:
                singular[name] = max(singular.get(name, -1.0), min(rel))
            else:
                regular[name] = min(regular.get(name, 1.0), min(rel))
    lo = min(regular, key=regular.get)
    hi = max(singular, key=singular.get)
    print("smallest regular pivot %.1e (%s); largest singular %.1e (%s)" % (regular[lo], lo, singular[hi], hi))
    assert regular[lo] >= 1e-8 and singular[hi] <= 1e-14


def test_gn6_on_random_lines(wm):
    """32 seeded lines of 500 collinear pairs, up to 35 m off the origin, moved by a few centimetres: J^T J has rank 5 up
    to the rounding of the float32 points.  The old rule went by the sign of a pivot at rounding level.  kGnPivotTol
    reports 31 of the 32; the one it lets pass (pivot 6e-11 of its entry: the points' own rounding, seen from a line
    that runs close to a coordinate axis) reaches the reference's residual, 2.6e-11 from 0.36.  Whichever way the flag
    falls: the step returned is finite and rigid; a reported system is NOT stepped (wm.HostIcp: WM_CONV_DEGENERATE, pose
    untouched, residual as it was), an unreported one lowers the residual.  The SVD step of the same pairs has all
    four properties."""
    rng = np.random.default_rng(1)
    reported = 0
    for k in range(32):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        p = (rng.uniform(-10, 10, 500)[:, None] * d + rng.uniform(-20, 20, 3)).astype(np.float32)
        q = (p.astype(np.float64) + [0.01, -0.02, 0.015]).astype(np.float32)
        d2 = ((p - q) ** 2).sum(1).astype(np.float32)
        st, _ = IR.sums(p, q, d2, IR.GN6)
        rel = _chol_pivots(st)
        rc, T = wm.gn6_from_stats(st)
        assert rc in (wm.WM_OK, wm.WM_NOT_CONVERGED) and np.isfinite(T).all()
        orth, det = IR.rigid_error(T)
        assert orth <= 1e-12 and det <= 1e-12
        h = wm.HostIcp(wm.icp_params(mode=wm.WM_ICP_GN6, max_iter=30))
        h.apply(st)
        got = h.get()
        before = IR.ssr(np.eye(4), p, q)
        if rc == wm.WM_NOT_CONVERGED:
            reported += 1
            assert min(rel) <= 1e-12
            assert got["done"] and not got["converged"] and got["state"] == "DEGENERATE" and got["iterations"] == 0
            assert np.array_equal(got["T"], np.eye(4)) and got["n_corr"] == 500 and got["rc"] == wm.WM_NOT_CONVERGED
        else:
            after = IR.ssr(T, p, q)
            print("line %d passes (smallest pivot %.1e of its entry): residual %.3e -> %.3e, reference %.3e" %
                  (k, min(rel), before, after, IR.ssr(IR.step(p, q, IR.GN6), p, q)))
            assert min(rel) > 1e-12 and after < before
            assert not got["done"] and got["iterations"] == 1 and np.array_equal(got["T"], T)
        st_svd, _ = IR.sums(p, q, d2, IR.SVD)
        rc, Ts = wm.umeyama_from_stats(st_svd)
        assert rc == wm.WM_OK
        Tr = IR.step(p, q, IR.SVD)
        # (both forms are free about the line: what separates them is the points' own distance from it, 2^-23 of 35 m)
        assert IR.disp(Ts, Tr, p) <= 2.0 * 35.0 * 2.0 ** -23
        _properties(Ts, Tr, p, q, 2.0 * 35.0 * 2.0 ** -23)
    print("singular systems reported: %d of 32" % reported)
    assert reported >= 31


@pytest.mark.parametrize("name", sorted(IR.FREE) + ["mirror", "mirror_thin"])
def test_host_icp_first_iteration_is_the_oracles(wm, oracle, name):
    """wm.HostIcp.apply (icp_apply_stats on the host) on the sums of the first search: the oracle's states and counts,
    forced and free-running, both modes"""
    c = IR.case(name)
    _, p, q, d2 = _pq(c, I4)
    for mode_name, mode in IR.MODES:
        st, _ = IR.sums(p, q, d2, mode)
        for kw in (dict(force_iterations=1), dict(max_iter=1), dict(max_iter=30)):
            h = wm.HostIcp(wm.icp_params(mode=mode, max_corr=c.max_corr, **kw))
            h.apply(st)
            got = h.get()
            want = oracle.icp_align(*c.finite(), max_corr=c.max_corr, mode=mode, incremental_float=0, **kw)
            assert got["n_corr"] == len(p)
            if want["iterations"] <= 1:  # (n_corr and mse are the last search's)
                assert got["n_corr"] == want["n_corr"] and abs(got["mse"] - want["mse"]) <= 1e-13 * got["mse"]
            if mode == IR.GN6 and name in IR.FREE:
                assert want["state"] == "DEGENERATE" and want["iterations"] == 0 and not want["converged"]
                assert got["state"] == "DEGENERATE" and got["iterations"] == 0 and not got["converged"] and got["done"]
                assert np.array_equal(got["T"], np.eye(4)) and np.array_equal(want["T"], np.eye(4))
                continue
            if "max_iter" in kw and kw["max_iter"] == 30:
                # one iteration of a longer run: not done (or done by a stopping rule the oracle's first iteration met too)
                assert got["done"] == (want["iterations"] == 1)
                if got["done"]:
                    assert got["state"] == want["state"]
                want = oracle.icp_align(*c.finite(), max_corr=c.max_corr, mode=mode, incremental_float=0, force_iterations=1)
            else:
                assert got["done"] and got["converged"] and got["state"] == want["state"]
            assert got["iterations"] == 1
            assert IR.disp(got["T"], want["T"], p) <= max(1e-9, 100.0 * (IR.REF_FORMS[name][mode] or 0.0)), (name, mode_name)
            orth, det = IR.rigid_error(got["T"])
            assert orth <= 1e-12 and det <= 1e-12


# ------------------------------------------------------------------- 55 km from the origin: what can be held there
FAR = ["utm", "utm_plane"]


@pytest.mark.parametrize("name", FAR)
def test_far_digits_are_lost_when_the_raw_sums_round(wm, name):
    """Would an error-free Sqp / n - qm pm^T in umeyama_from_stats bring the far cases' paths together?  No: the digits go
    when the raw sums are ROUNDED TO DOUBLE (Sqp is 1e13 there, its ulp 2e-3), before the solve sees them.  sigma formed
    in long double from the correctly rounded sums -- an exact solve -- is 7e-10 ... 3.5e-9 m from the centred reference,
    the library 2.3e-9 ... 1.2e-8: a factor of three at the most, and two device paths, whose sums differ by a few ulps,
    stay about 1e-8 m (1e-9 rad) apart after a step whatever the solve does."""
    c = IR.case(name)
    for Tf in (c.T0f, I4):
        _, p, q, d2 = _pq(c, Tf)
        rc, T_lib, st = _lib_step(wm, p, q, d2, IR.SVD)
        n = LD(st[0])
        pm, qm = st[1:4].astype(LD) / n, st[4:7].astype(LD) / n
        sigma = (st[7:16].astype(LD).reshape(3, 3) / n - np.outer(qm, pm)).astype(np.float64)
        U, _, Vt = np.linalg.svd(sigma)
        R = U @ np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0]) @ Vt
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, (qm - R.astype(LD) @ pm).astype(np.float64)
        ref = IR.step(p, q, IR.SVD)
        exact, lib = IR.disp(T, ref, p), IR.disp(T_lib, ref, p)
        print("%s: exact solve on the rounded sums %.2e m, library %.2e m, ulp of Sqp %.1e" % (name, exact, lib, np.spacing(np.abs(st[7:16]).max())))
        assert exact >= 0.1 * lib and exact >= 5e-10


@pytest.mark.parametrize("name", FAR + ["scene"])
def test_far_registrations_scatter_by_the_float_pose(oracle, name):
    """IR.float_pose_floor held by experiment, on the reference alone.  IR.icp_loop (PCL's loop around step(SVD)) is run
    as it is and eight times with the pose turned by 1e-9 rad about the cloud's centroid after the first step -- 1.5e-8 m
    over the cloud, what two device paths are apart after one step 55 km out.  Measured there: six forced iterations end
    3.5e-4 ... 2.2e-3 m apart, free-running registrations 3.6e-4 ... 3.9e-3 m, after 12 to 30 iterations where the
    unperturbed one takes 28 (utm) and 16 (utm_plane), by REL_MSE or by the iteration limit; pose_error between them
    reads decimetres.  The last search's correspondences do NOT change; the mean squared distance, at the float32 points'
    own floor (1e-6 ... 1e-5 m^2), varies more than tenfold with the roundings the float pose happens to take.  `scene`, 50 m from the origin, keeps its iteration count and ends 1.4e-7 m apart at the most.
    So at 55 km the iteration count, the state and a pose within helpers.TOL_T cannot be held against another run of the
    SAME algorithm; the correspondences, the states' kind and disp within IR.float_pose_floor can (tests/test_icp_stress_gpu.py)."""
    c = IR.case(name)
    src, tgt = c.finite()
    tree = oracle.KdTree(tgt)
    cen = src.astype(np.float64).mean(0)
    floor = IR.float_pose_floor(c)
    base6, basef = IR.icp_loop(c, tree.nn, force=6), IR.icp_loop(c, tree.nn)
    want = oracle.icp_align(src, tgt, max_corr=c.max_corr, max_iter=30, incremental_float=0)
    assert (basef[1], basef[2]) == (want["iterations"], want["state"])  # (the loop is the oracle's)
    rng = np.random.default_rng(7)
    six, free, its, dts, mses = [], [], [], [], [basef[4]]
    for k in range(8):
        w = rng.normal(size=3)
        w *= 1e-9 / np.linalg.norm(w)
        P = np.eye(4)
        P[:3, :3] = IR.rodrigues(w)
        P[:3, 3] = cen - P[:3, :3] @ cen
        r6, rf = IR.icp_loop(c, tree.nn, P, force=6), IR.icp_loop(c, tree.nn, P)
        assert np.array_equal(r6[3], base6[3]) and np.array_equal(rf[3], basef[3])
        six.append(IR.disp(r6[0], base6[0], src))
        free.append(IR.disp(rf[0], basef[0], src))
        its.append(rf[1])
        dts.append(pose_error(rf[0], basef[0])[0])
        assert rf[2] in (("REL_MSE", "ITERATIONS") if c.far else (basef[2],))
        mses.append(rf[4])
    print("%s: six iterations %.1e ... %.1e m, free-running %.1e ... %.1e m after %d ... %d iterations (unperturbed %d), "
          "pose_error up to %.1e m, mse %.1e ... %.1e; allowed %.1e" % (name, min(six), max(six), min(free), max(free), min(its), max(its), basef[1],
                                                                       max(dts), min(mses), max(mses), floor))
    assert max(six + free) <= floor
    if c.far:
        assert max(six + free) > 10 * TOL_T and max(dts) > 10 * TOL_T and len(set(its)) > 1
    else:
        assert set(its) == {basef[1]} and max(six + free) <= 1e-6
