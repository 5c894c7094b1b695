"""ICP after its search on stress cases (tests/icp_reference.py): every kernel that forms an iteration's 17 sums and
takes the step -- k_icp_stats and its row reduction, the filtered sums of the rejection path, the fused search with
bins and with rows, the brute-force search, the certificate kernel (k_nn_cert's hand-scheduled copy of the terms), the
resident kernel, the one-workgroup batch kernel -- against a plain numpy reference AND the oracle, on collinear and
coincident pairs, an exact plane, a mirrored target, three pairs in a row, clouds 55 km from the origin, coordinates of
centimetres, a pair exactly on the distance gate, 0 / 1 / 3 / 4 pairs, non-finite rows on both sides, and cloud sizes AND
numbers of contributing lanes around the 64-lane wave, kBlock = 256 and kSmThreads = 1024.

Metric: IR.disp, the largest distance between two poses' images of the points -- defined where a pose difference is not
(the FREE cases).  Bounds: the sums within 1e-13 x sum |term| of the correctly rounded (fsum) value; a step within
max(1e-9 m, 100 x IR.REF_FORMS) of the reference step; outside FREE also within 1e-7 m / 1e-8 rad of the oracle
(test_icp_gpu.py's figure) unless the case sits in LOOSE.

Not reached by clouds of at most 3 375 points: k_icp_small's HBM variant (targets above 10 000 points; test_batch_gpu.py
has those); and k_reduce_rows never adds more than 14 rows of partial sums (3 375 points are 14 workgroups of 256).

Worst figures measured on an MI355X (this file prints them with -s), per case group:
    case group                                  sums: |err| / sum|term|   first step: disp from    six iterations: disp
                                                (stats_for and reject)    the reference step [m]   between paths [m]
    exact_plane, noisy_plane, shell, lattice    2.4e-16                   8.9e-15                  1.5e-14
    scene, holes, holes_both, half, half_start  2.4e-16                   4.5e-14                  6.7e-14
    clumps_outliers, dups                       2.4e-16                   3.9e-13                  5.8e-13
    mirror, mirror_thin, mm                     2.3e-16                   2.1e-14                  1.8e-14
    three_pairs, four_pairs, collinear3         0 ... 2.4e-16             6.9e-13                  2.4e-13
    n10 ... n1025                               2.4e-16                   3.0e-14                  2.0e-14
    pairs63 ... pairs1025                       2.4e-16                   5.7e-14                  6.1e-14
    line, line_x, point (SVD)                   2.4e-16                   4.5e-15                  3.7e-7 (line; allowed 6.6e-6)
    line_diag, line_far (SVD)                   1.8e-16                   4.0e-7 (allowed 1.5e-5)  2.8e-6 (allowed 6.6e-6)
    utm, utm_plane (55 km out)                  2.4e-16                   2.3e-8 (allowed 2.6e-7)  3.5e-3 (allowed 1.0e-2)
Every path of the first-step test ran on every case with at least three pairs (its counter is asserted); with cert_from
= 1 the certificate kernel ran five of the six iterations on every case, launched and resident; by its own policy (-1)
it ran 2 or 3 of the six, except on line, line_x, line_diag, line_far, collinear3, clumps_outliers and mirror, where the
steps never became small enough within six iterations.  Free-running registrations: every case off the `far` ones
equals the oracle's status, state, iterations and n_corr on both paths, T to 2e-14 m / 2e-14 rad.  The `far` ones end
within 3.9e-3 m of the oracle over the points (allowed 1.0e-2) while pose_error reads 0.02 ... 0.43 m / 3e-7 ... 8e-6 rad:
the lever of 55 km; the last search's correspondences equal the oracle's on both of them, in both modes (0 rows differ).

What this file found.  The KERNELS are sound: every path forms the sums of the reference to 2.4e-16 of sum |term| --
three decades inside the bound -- with unmatched and non-finite lanes inside contributing waves, on every edge in the
number of pairs and of points; k_nn_cert's hand-scheduled copy of the terms, the resident kernel and the one-workgroup
kernel take the reference's step to 1e-13 m.  What was wrong sits behind them, in the shared solve, and showed on the CPU
first (tests/test_icp_reference_cpu.py): gn6_from_stats on a singular J^T J (collinear or coincident pairs) RAISED the
residual -- `point` 0.15 -> 1.1e8, `collinear3` 0.53 -> 2.8e13, `line_far` 5.2 -> 5.6e4 -- because chol_solve's report was
ignored and, where the pivot came out positive at rounding level, not even made.  Fixed in csrc/wm_math.hpp
(kGnPivotTol: a pivot at or below 1e-12 of its own diagonal entry is singular) and csrc/wm_icp_step.hpp (icp_apply_stats
ends the registration WM_CONV_DEGENERATE, pose untouched), which every path shares; the oracle states the same rule.
The SVD step is well defined on the same input and registers it on every path.  Two things are as they were:
  * 55 km from the origin (`far`) umeyama_from_stats keeps the points to 2e-8 m in one step (Sqp / n - qm pm^T from
    numbers of 3e9) -- inside 100 x IR.REF_FORMS, and up to 9e-5 m of pose_error's translation, which is the rotation
    difference (1.6e-9 rad) times 55 km: utm and utm_plane sit in LOOSE for the one-step comparison with the oracle.  After
    several iterations two paths, and the oracle, end up to 3.5e-3 m apart there, because the searches run under PCL's FLOAT
    pose, whose entries weigh 3 mm at that distance.  tests/test_icp_reference_cpu.py shows both on the CPU: the
    reference loop lands up to 3.9e-3 m, 12 to 30 iterations and 0.35 m of pose_error from a run of itself whose pose
    was turned by 1e-9 rad (test_far_registrations_scatter_by_the_float_pose) -- so in parts c and d the two LOOSE cases
    are held to IR.float_pose_floor over the points, to equal counts, to correspondences within two rows of each other and
    of the oracle, and to a stopping state of the kind that experiment shows, not to TOL_T or an iteration count -- and an
    error-free sigma would NOT bring the paths together (test_far_digits_are_lost_when_the_raw_sums_round: the
    digits go when Sqp, 1e13 with an ulp of 2e-3, is rounded to double; an exact solve on those sums gains a factor of
    three at the most).  Keeping them would take centred sums, a change to every kernel above: not made here.
  * GN6 linearises the rotation about the origin: from the identity on utm the exact step leaves 0.38 m per point and
    raises the residual (17.7 -> 301), on the device as in the reference; the next iterations recover.
Nearest-neighbour pairing defeats `mirror` (sigma keeps a positive determinant); `mirror_thin` reaches Umeyama's
reflection branch and comes back rigid on every path.
"""
import math

import numpy as np
import pytest

import icp_reference as IR
from helpers import TOL_R, TOL_T, pose_error

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32)
SUM_TOL = 1e-13   # of sum |term|: a thread adds fewer than a hundred terms, six halvings and the rows follow, each rounding
#                   once at 2^-53 -- about 1.2e-14 -- and one digit of margin
MSE_TOL = 1e-13   # relative, of fsum(d2) / n
STEP_FLOOR = 1e-9  # metres: what test_batch_gpu.py allows two device paths that add the same pairs in another order
ORACLE_T, ORACLE_R = 1e-7, 1e-8  # test_icp_gpu.py::test_icp_forced_iterations_match_oracle
# Cases held to helpers.TOL_T / TOL_R against the ORACLE's pose instead of 1e-7 m / 1e-8 rad after ONE step, and after
# several iterations to what _hold_far states.  At most two.
LOOSE = {
    # 55 km from the origin pose_error's translation is the rotation difference times 55 km: umeyama_from_stats forms
    # sigma as Sqp / n - qm pm^T from numbers of 3e9 and keeps the rotation to about 1e-9 rad there (IR.REF_FORMS: 1.2e-8 m
    # over the cloud), which is 5e-5 m of translation.  The points themselves agree to IR.REF_FORMS -- the disp
    # bound is NOT loosened.
    "utm": "one step, worst path: 5.4e-5 m / 9.7e-10 rad against the oracle, 2.0e-8 m over the points",
    "utm_plane": "one step, worst path: 9.0e-5 m / 1.6e-9 rad against the oracle, 2.3e-8 m over the points",
}
DEFAULTS = {"cert_from": -1, "late": 0, "bins": 1}
BINS_PATHS = ("fused+bins", "certificate")  # the paths of _paths() whose sums go through the bins (wm_bins.hpp)

_first = {}


def _load(ctx, c):
    ctx.set_source(c.src)
    ctx.set_target(c.tgt)


def _options(ctx, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        ctx.set_option(k, v)


def _pq(c, Tf):
    idx, d2 = c.pairs_at(Tf)
    si, p, q = IR.matched(c.src, c.tgt, Tf, idx)
    return idx, si, p, q, d2[si]


def _first_step(oracle, name):
    """what the first iteration of a registration of the case must give: the pairs under the identity, the mean d2, the
    reference step and the oracle's one forced iteration, per mode -- computed once"""
    if name not in _first:
        c = IR.case(name)
        idx, si, p, q, d2 = _pq(c, I4)
        r = dict(idx=idx, n=len(si), p=p, q=q, mse=math.fsum(d2.astype(np.float64)) / len(si) if len(si) else 0.0, step={}, oracle={})
        for _, mode in IR.MODES:
            if len(si) >= 3:
                r["step"][mode] = IR.step(p, q, mode)
            r["oracle"][mode] = oracle.icp_align(*c.finite(), max_corr=c.max_corr, force_iterations=1, mode=mode, incremental_float=0)
        _first[name] = r
    return _first[name]


def _degenerate(name, mode):
    return mode == IR.GN6 and name in IR.FREE


def _hold_to_oracle(name, T, T_oracle, what):
    dt, ang = pose_error(T, T_oracle)
    tol = (TOL_T, TOL_R) if name in LOOSE else (ORACLE_T, ORACLE_R)
    print("    %s against the oracle: %.2e m %.2e rad%s" % (what, dt, ang, " (LOOSE)" if name in LOOSE else ""))
    assert dt <= tol[0] and ang <= tol[1], (name, what, dt, ang)


def _four_properties(T, T_ref, p, q, delta):
    assert np.isfinite(T).all()
    orth, det = IR.rigid_error(T)
    assert orth <= 1e-12 and det <= 1e-12, (orth, det)
    before, after, ref = IR.ssr(np.eye(4), p, q), IR.ssr(T, p, q), IR.ssr(T_ref, p, q)
    assert after <= before and after <= ref + IR.ssr_slack(delta, T_ref, p, q), (before, after, ref)


# --------------------------------------------------------------------------- a / e. the sums, where they can be read
def _yaw_about_centroid(c, angle):
    cen = IR.finite_src(c).astype(np.float64).mean(0)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]
    T[:3, 3] = cen - T[:3, :3] @ cen
    return T.astype(np.float32)


@pytest.mark.parametrize("name", IR.NAMES)
def test_sums_match_the_rounded_reference(wm, ctx, name):
    """nn_search at the pairing pose, then the sums through wm_icp_stats_for (k_icp_stats + the row reduction) and through
    wm_icp_reject with a rule that rejects nothing (the filtered sums), SVD and GN6: n equal, every other component
    within 1e-13 x sum |term| of the fsum value.  (Neither path goes through the bins: no floor for `mm`.)"""
    c = IR.case(name)
    _load(ctx, c)
    poses = [("T0f", c.T0f)] + ([("yaw 0.3 rad", _yaw_about_centroid(c, 0.3))] if name == "utm" else [])
    failures = []
    for pose_name, Tf in poses:
        idx, si, p, q, d2 = _pq(c, Tf)
        T = Tf.astype(np.float64)
        gi, gd = ctx.nn_search(T, c.max_corr, wm.WM_NN_GRID)
        assert np.array_equal(gi, idx) and np.array_equal(gd[si], d2), (name, pose_name, int((gi != idx).sum()))
        worst = {}
        for mode_name, mode in IR.MODES:
            want, scale = IR.sums(p, q, d2, mode)
            rej = ctx.icp_reject(T, mode=mode, reject=wm.WM_REJECT_TRIMMED, ratio=1.0)
            assert rej["n_matched"] == rej["n_kept"] == len(si) and np.array_equal(rej["kept"], idx >= 0), (name, rej["n_matched"], rej["n_kept"])
            for path, got in (("stats_for", ctx.icp_stats_for(T, mode)), ("reject", rej["stats"])):
                assert got[0] == want[0] == len(si), (name, path, got[0])
                err = np.abs(got[:29] - want[:29])
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(scale[:29] > 0, err / scale[:29], np.where(err > 0, np.inf, 0.0))
                worst[(mode_name, path)] = float(ratio.max())
                if not (ratio <= SUM_TOL).all():
                    failures.append((pose_name, mode_name, path, int(ratio.argmax()), float(ratio.max())))
        print("SUMS %s %s (%d pairs): " % (name, pose_name, len(si)) + "  ".join("%s/%s %.1e" % (k[0], k[1], v) for k, v in sorted(worst.items())))
    assert not failures, failures


# ------------------------------------------------------------- b. one step, on every path that forms the sums itself
def _paths(wm):
    """(name, options, icp_align keywords, the counter that shows the path ran)"""
    grid = dict(nn_method=wm.WM_NN_GRID)
    return [
        ("fused+bins", {}, grid, lambda r: r["nn_levels"] > 0 and r["cert_launches"] == 0),
        ("fused+rows", {"bins": 0}, grid, lambda r: r["nn_levels"] > 0 and r["cert_launches"] == 0),
        ("brute", {}, dict(nn_method=wm.WM_NN_BRUTE), lambda r: r["nn_levels"] == 0),
        ("reject", {}, dict(reject=wm.WM_REJECT_TRIMMED, reject_ratio=1.0, **grid), lambda r: r["n_matched"] == r["n_corr"]),
        ("certificate", {"cert_from": 0}, grid, lambda r: r["cert_launches"] == 1 and r["late_iterations"] == 0),
        ("resident", {"cert_from": 0, "late": 1}, grid, lambda r: r["late_iterations"] == 1),
    ]


def _check_first_step(wm, name, mode, path, r, ref, oracle_step, worst):
    c = IR.case(name)
    n = ref["n"]
    if n < 3:
        assert r["rc"] == wm.WM_TOO_FEW and r["state"] == "NO_CORRESPONDENCES" and r["T"] is None, (name, path, r["rc"], r["state"])
        assert r["n_corr"] == n
        return
    assert r["n_corr"] == n, (name, path, r["n_corr"], n)
    # (`mm` through the bins: a wave's partial sum of d2 is truncated at 2^-56, once per wave)
    floor = -(-n // 64) * 2.0 ** -56 / n if name == "mm" and path in BINS_PATHS else 0.0
    assert abs(r["mse"] - ref["mse"]) <= MSE_TOL * ref["mse"] + floor, (name, path, r["mse"], ref["mse"])
    if _degenerate(name, mode):
        assert r["rc"] == wm.WM_NOT_CONVERGED and r["state"] == "DEGENERATE" and r["T"] is None and r["iterations"] == 0, (name, path, r["rc"], r["state"])
        assert oracle_step["state"] == "DEGENERATE"
        return
    assert r["rc"] == wm.WM_OK and r["state"] == "FORCED" and r["iterations"] == 1, (name, path, r["rc"], r["state"])
    T = r["T"]
    form = IR.REF_FORMS[name][mode]
    d = IR.disp(T, ref["step"][mode], IR.compare_points(c, I4, ref["p"]))
    worst[(path, mode)] = d
    assert d <= max(STEP_FLOOR, 100.0 * form), (name, path, mode, d)
    if name in IR.FREE:
        _four_properties(T, ref["step"][mode], ref["p"], ref["q"], max(STEP_FLOOR, 100.0 * form))
    else:
        _hold_to_oracle(name, T, oracle_step["T"], "%s mode %d" % (path, mode))


@pytest.mark.parametrize("name", IR.NAMES)
def test_first_step_on_every_path(wm, ctx, oracle, name):
    """icp_align(force_iterations = 1): T is the first step from the identity.  Fused search with bins and with rows,
    brute-force search + k_icp_stats, the rejection path's filtered sums, k_nn_cert and the resident kernel from iteration
    0 (no bounds yet: every query searched, the sums their own), the one-workgroup kernel alone and as the middle item of
    three.  Each path's counter shows that it ran."""
    c = IR.case(name)
    ref = _first_step(oracle, name)
    _load(ctx, c)
    worst = {}
    try:
        for mode_name, mode in IR.MODES:
            for path, opts, kw, ran in _paths(wm):
                _options(ctx, **opts)
                r = ctx.icp_align(max_corr=c.max_corr, force_iterations=1, mode=mode, carry_state=0, **kw)
                if ref["n"] >= 3 and not _degenerate(name, mode):
                    assert ran(r), (name, path, {k: r[k] for k in ("nn_levels", "cert_launches", "late_iterations", "n_matched", "n_corr")})
                gi, _ = ctx.correspondences()
                assert np.array_equal(gi, ref["idx"]), (name, path, int((gi != ref["idx"]).sum()))
                _check_first_step(wm, name, mode, path, r, ref, ref["oracle"][mode], worst)
            _options(ctx)
            n65, scene = IR.case("n65"), IR.case("scene")
            # (the batch kernel is shown to have run by its status alone: with res <= 0 and a target below 65 535 points
            # wm_icp_batch_match has no other path to a result for SVD / GN6 without rejection)
            alone = ctx.icp_batch_match([(c.src, c.tgt)], with_info=False, max_corr=c.max_corr, force_iterations=1, mode=mode)
            three = ctx.icp_batch_match([(n65.src, n65.tgt), (c.src, c.tgt), (scene.src, scene.tgt)], with_info=False,
                                        max_corr=c.max_corr, force_iterations=1, mode=mode)
            _check_first_step(wm, name, mode, "batch alone", alone[0], ref, ref["oracle"][mode], worst)
            _check_first_step(wm, name, mode, "batch middle", three[1], ref, ref["oracle"][mode], worst)
            assert three[1]["rc"] == alone[0]["rc"] and (three[1]["T"] is None or np.array_equal(three[1]["T"], alone[0]["T"]))
            assert three[0]["rc"] in (wm.WM_OK, wm.WM_TOO_FEW) and three[2]["rc"] in (wm.WM_OK, wm.WM_TOO_FEW)  # (at THIS case's max_corr)
    finally:
        _options(ctx)
    if worst:
        print("STEP %s (%d pairs): worst disp from the reference step %.1e m (%s); allowed svd %.1e gn6 %s" % (
            name, ref["n"], max(worst.values()), max(worst, key=worst.get), max(STEP_FLOOR, 100 * IR.REF_FORMS[name][0]),
            "-" if IR.REF_FORMS[name][1] is None else "%.1e" % max(STEP_FLOOR, 100 * IR.REF_FORMS[name][1])))


# ------------------------------------------------ c. several steps: the certificate kernel and the resident loop
def _between_paths(c):
    """the disp allowed between two device paths after SEVERAL iterations: 1e-9 m (test_batch_gpu.py: the same pairs added
    in another order) -- except where a derivation says more: the FREE cases (IR.line_floor: the free rotation about the
    pairs' line is decided by the points' rounding, anew in every iteration) and the two LOOSE ones, 55 km out
    (IR.float_pose_floor, held by tests/test_icp_reference_cpu.py::test_far_registrations_scatter_by_the_float_pose: the
    reference loop itself ends up to 3.9e-3 m from a run whose pose was turned by 1e-9 rad; measured here 3.5e-3 m)"""
    if c.name in LOOSE:
        return IR.float_pose_floor(c)
    return max(STEP_FLOOR, IR.line_floor(c)) if c.name in IR.FREE and c.name != "point" else STEP_FLOOR


def _corr_mismatch(c, gi, want_idx):
    """rows of the caller's source whose match differs from the oracle's (which indexes the finite target)"""
    fs, ft = np.nonzero(np.isfinite(c.src).all(1))[0], np.nonzero(np.isfinite(c.tgt).all(1))[0]
    return int((gi[fs] != np.where(want_idx >= 0, ft[np.maximum(want_idx, 0)], -1)).sum())


def _hold_far(c, T, T_oracle, what):
    """a LOOSE case after SEVERAL iterations against the oracle: the images of the points within IR.float_pose_floor.
    helpers.TOL_T / TOL_R, what LOOSE means for one step, cannot be met here by ANY implementation: the searches run
    under PCL's float pose, and test_far_registrations_scatter_by_the_float_pose (CPU) shows the reference loop itself
    landing 3.9e-3 m -- and 0.35 m of pose_error, whose translation is the rotation difference times 55 km -- from a run
    of itself whose pose was turned by 1e-9 rad, the distance of two device paths after one step.  What that experiment
    finds unchanged is asserted by the callers: the correspondences, the count, the kind of stopping state."""
    d = IR.disp(T, T_oracle, IR.finite_src(c))
    print("    %s against the oracle: disp %.2e m (allowed %.1e), pose_error %.2e m %.2e rad" % ((what, d, IR.float_pose_floor(c)) + pose_error(T, T_oracle)))
    assert d <= IR.float_pose_floor(c), (c.name, what, d)


SIX = [n for n in IR.NAMES if n not in ("no_pair", "one_pair")]


@pytest.mark.parametrize("name", SIX)
def test_six_forced_iterations_agree_on_every_path(wm, ctx, oracle, name):
    """force_iterations = 6 with the certificate kernel never (-2), from iteration 1, by its policy (-1), each launched
    and resident, plus the batch: one n_corr, the same final correspondences, the same pose to 1e-9 m; outside FREE the
    oracle's pose, count and correspondences (two may differ, as test_correspondences_after_align_match_oracle allows)."""
    c = IR.case(name)
    _load(ctx, c)
    src = IR.finite_src(c)
    try:
        for mode_name, mode in IR.MODES:
            if _degenerate(name, mode):
                continue
            runs = {}
            for cert_from in (-2, 1, -1):
                for late in (0, 1):
                    _options(ctx, cert_from=cert_from, late=late)
                    r = ctx.icp_align(max_corr=c.max_corr, force_iterations=6, mode=mode, carry_state=0, nn_method=wm.WM_NN_GRID)
                    r["corr"] = ctx.correspondences()[0]
                    runs[(cert_from, late)] = r
            _options(ctx)
            base = runs[(-2, 0)]
            assert base["rc"] == wm.WM_OK and base["iterations"] == 6 and base["cert_launches"] == 0 and base["late_iterations"] == 0
            assert runs[(-2, 1)]["cert_launches"] == 0 and runs[(-2, 1)]["late_iterations"] == 0
            # forced from iteration 1: five certificate launches, all five inside the resident kernel when it is on
            assert runs[(1, 0)]["cert_launches"] == 5 and runs[(1, 0)]["late_iterations"] == 0, (name, runs[(1, 0)]["cert_launches"])
            assert runs[(1, 1)]["cert_launches"] == 5 and runs[(1, 1)]["late_iterations"] == 5, (name, runs[(1, 1)]["late_iterations"])
            print("SIX %s %s: policy (-1) ran %d certificate launches, %d of them resident" % (
                name, mode_name, runs[(-1, 0)]["cert_launches"], runs[(-1, 1)]["late_iterations"]))
            worst = 0.0
            for key, r in runs.items():
                assert r["rc"] == wm.WM_OK and r["n_corr"] == base["n_corr"], (name, key, r["rc"], r["n_corr"], base["n_corr"])
                # (LOOSE: the last searches ran under float poses a rounding apart -- two rows may differ, the count
                # test_correspondences_after_align_match_oracle allows against the oracle for the same reason)
                diff = int((r["corr"] != base["corr"]).sum())
                assert diff <= (2 if name in LOOSE else 0), (name, key, diff)
                worst = max(worst, IR.disp(r["T"], base["T"], src))
            batch = ctx.icp_batch_match([(c.src, c.tgt)], with_info=False, max_corr=c.max_corr, force_iterations=6, mode=mode)[0]
            assert batch["rc"] == wm.WM_OK and batch["n_corr"] == base["n_corr"]
            worst = max(worst, IR.disp(batch["T"], base["T"], src))
            allowed = _between_paths(c)
            print("SIX %s %s: worst disp between paths %.1e m (allowed %.1e)" % (name, mode_name, worst, allowed))
            assert worst <= allowed, (name, mode_name, worst)
            if name in IR.FREE:
                orth, det = IR.rigid_error(base["T"])
                assert orth <= 1e-12 and det <= 1e-12
                continue
            want = oracle.icp_align(*c.finite(), max_corr=c.max_corr, force_iterations=6, mode=mode, incremental_float=0, want_corr=True)
            assert base["n_corr"] == want["n_corr"]
            if name in LOOSE:
                _hold_far(c, base["T"], want["T"], "six iterations " + mode_name)
            else:
                _hold_to_oracle(name, base["T"], want["T"], "six iterations " + mode_name)
            mism = _corr_mismatch(c, base["corr"], want["corr_idx"])
            assert mism <= 2, (name, mode_name, mism)
    finally:
        _options(ctx)


# ------------------------------------------------------------------------------------ d. free-running registrations
@pytest.mark.parametrize("name", IR.NAMES)
def test_free_running_registrations(wm, ctx, oracle, name):
    """max_iter = 30 under the default stopping rules, one pair and the batch.  Outside FREE: the oracle's status,
    state, iterations and n_corr, its pose to 1e-7 m / 1e-8 rad (LOOSE: helpers.TOL_T / TOL_R).  FREE: both paths and the
    oracle agree on status and state, T is finite and rigid, the mean squared distance does not rise."""
    c = IR.case(name)
    ref = _first_step(oracle, name)
    _load(ctx, c)
    for mode_name, mode in IR.MODES:
        one = ctx.icp_align(max_corr=c.max_corr, max_iter=30, mode=mode, carry_state=0)
        one_corr = ctx.correspondences()[0]
        batch = ctx.icp_batch_match([(c.src, c.tgt)], with_info=False, max_corr=c.max_corr, max_iter=30, mode=mode)[0]
        want = oracle.icp_align(*c.finite(), max_corr=c.max_corr, max_iter=30, mode=mode, incremental_float=0, want_corr=True)
        want_rc = wm.WM_OK if want["converged"] else (wm.WM_TOO_FEW if want["state"] == "NO_CORRESPONDENCES" else wm.WM_NOT_CONVERGED)
        print("FREE-RUN %s %s: one pair %s, batch %s, oracle %s" % (name, mode_name, *(
            "rc %d %s it %d n %d mse %.3e" % (g["rc"], g["state"], g["iterations"], g["n_corr"], g["mse"]) for g in (one, batch, dict(want, rc=want_rc)))))
        for path, g in (("one pair", one), ("batch", batch)):
            # (LOOSE: REL_MSE or the iteration limit, whichever the roundings bring first -- see below)
            states = ("REL_MSE", "ITERATIONS") if name in LOOSE else (want["state"],)
            assert g["rc"] == want_rc and g["state"] in states and want["state"] in states, (name, mode_name, path, g["rc"], g["state"], want["state"])
            assert (g["T"] is None) == (want_rc != wm.WM_OK)
            if name in IR.FREE:
                if g["T"] is not None:
                    orth, det = IR.rigid_error(g["T"])
                    assert np.isfinite(g["T"]).all() and orth <= 1e-12 and det <= 1e-12
                    assert g["mse"] <= ref["mse"] * (1.0 + MSE_TOL), (name, path, g["mse"], ref["mse"])
                continue
            if name in LOOSE:
                # the float32 points are 4 mm apart and the mean squared distance sits at that floor: which iteration's
                # change first falls below fit_eps goes by roundings.  Measured on utm: 27, 9 and 28 iterations for the
                # one-pair path, the batch and the oracle; the reference loop against itself, pose turned by 1e-9 rad: 12 to
                # 30 (test_far_registrations_scatter_by_the_float_pose).  The count is not held; the result, the number of
                # pairs and -- where they can be read -- the last search's correspondences are
                assert g["n_corr"] == want["n_corr"] and 1 <= g["iterations"] <= 30
                _hold_far(c, g["T"], want["T"], "free-running %s %s" % (path, mode_name))
                if path == "one pair":
                    mism = _corr_mismatch(c, one_corr, want["corr_idx"])
                    print("    last search against the oracle's: %d rows differ" % mism)
                    assert mism <= 2, (name, mode_name, mism)
                continue
            assert (g["iterations"], g["n_corr"]) == (want["iterations"], want["n_corr"]), (name, mode_name, path, g["iterations"], want["iterations"])
            if g["T"] is not None:
                _hold_to_oracle(name, g["T"], want["T"], "free-running %s %s" % (path, mode_name))
        if one["T"] is not None:
            d = IR.disp(one["T"], batch["T"], IR.finite_src(c))
            print("    one pair against batch: disp %.2e m (allowed %.1e)" % (d, _between_paths(c)))
            assert d <= _between_paths(c), (name, mode_name, d)
