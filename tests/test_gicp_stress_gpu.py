"""GICP after its covariances on stress cases (tests/gicp_reference.py): k_gicp_mahal, k_gicp_fdf, k_gicp_quad and their
reductions, the resident evaluator, the host loop of wm_gicp_align with its status codes, and the batched gs_* kernels --
against the oracle AND against a plain numpy reference, on degenerate neighbourhoods (a point, a line, an exact plane,
duplicates, a lattice), clouds 55 km from the origin, unmatched pairs inside the stream (one of them exactly on the
distance gate: under the evaluation's pairing pose in `half`, under a registration's first search in `half_start`), 0, 1,
3 and 4 pairs, non-finite rows on both sides, and source sizes around the 64-lane wave and the
256-thread workgroup.

Both references are given the DEVICE's covariances (ctx.gicp_covariances: held to brute force by test_knn_stress_gpu.py),
so that what is compared is what comes after them.  Tolerances: test_gicp_gpu.py's against the oracle -- 1e-12 of |f|,
1e-10 of the largest gradient entry --; against the numpy reference the larger of that and 100 times the reference's own
distance from the oracle (GR.REF_VS_ORACLE_*: the margin for the device's summation order and libm, as for NDT), which
is the same 1e-12 / 1e-10 on every case since the oracle sits within last bits of the reference everywhere.

Worst differences measured on an MI355X over a case's three states (this file prints them with -s), relative as
above, f / gradient; the two objectives are within a few 1e-16 of each other on every case, the larger is given:
    case group                                        GPU against oracle       GPU against numpy reference
    exact_plane, noisy_plane, line, point             0       / 5.4e-17        2.1e-16 / 2.2e-16
    utm, utm_plane (55 km out)                        2.5e-16 / 1.3e-15        2.5e-16 / 1.3e-15
    shell, scene, holes, holes_both, half, half_start 8.3e-16 / 1.2e-15        1.0e-15 / 1.1e-15
    dups                                              1.2e-15 / 3.8e-15        1.2e-15 / 3.8e-15
    lattice, clumps_outliers                          1.2e-14 / 1.5e-14        1.2e-14 / 1.5e-14
    one_pair, three_pairs, four_pairs                 3.8e-16 / 2.7e-16        1.9e-16 / 3.6e-16
    n10 ... n1025                                     1.5e-15 / 1.4e-15        1.5e-15 / 1.5e-15
(the 1e-14 of lattice and clumps_outliers is the Mahalanobis matrix: both references are given the long double adjugate's
matrices, the device forms its own by cofactors in double -- the oracle is as far from the device there as the numpy
reference is.)

Whole registrations: EVERY case equals the oracle's -- status, pairs, outer and inner iterations, evaluations, f and T bit
for bit, both objectives, exact_plane's 100 outer iterations and 760 evaluations under the per-pair objective
included --, so no case is held to include/wavematch.h's looser 1e-6 m / 1e-6 rad (LOOSE is empty).  four_pairs
converges in the oracle (PCL needs four pairs, and has them), so its status is WM_OK and it has a T.

What this file found: the batched path matched NOTHING on `point` (WM_TOO_FEW_CORRESPONDENCES where the one-pair path and
the oracle register 500 pairs) -- knn_search capped its radius at the grid's own size, counted from a query inside the
grid, and the target's grid there is one cell of 16 um with the query 5 cm (3 000 cells) outside it; any small, tight
target farther than its own extent from the source was affected.  Fixed in csrc/wm_gicp_dev.hpp (knn_search<K, OUTSIDE>).
"""
import ctypes as C

import numpy as np
import pytest

import gicp_reference as GR
from helpers import pose_error
from test_gicp_batch_gpu import _same

pytestmark = pytest.mark.gpu

OBJECTIVES = [("statistics", 1, 1), ("pcl_sums", 0, 0)]  # (name, wm_gicp_params::objective, oracle objective mode)
F_TOL, G_TOL = 1e-12, 1e-10  # test_gicp_gpu.py::test_gicp_objective_and_gradient_match_oracle
BLOCKS = (1, 2, 13, 14, 19, 20, 4096)
KNOB_CASES = ["half", "utm", "clumps_outliers", "dups", "lattice"] + ["n%d" % n for n in GR.SIZES]
WORKGROUP = 256  # kBlock of csrc/wm_gicp.hip: an evaluation leaves min(ceil(n_src / 256), gicp_blocks) rows of partial sums


def _rows(name, nb):
    c = GR.case(name)
    return min(-(-int(np.isfinite(c.src).all(1).sum()) // WORKGROUP), nb)


# registrations that may differ from the oracle's by a last-bit libm difference taking a line-search branch
# (include/wavematch.h documents it for the batch): held to 1e-6 m / 1e-6 rad instead of equality.  At most two.
LOOSE = {}
_refs, _aligned = {}, {}


@pytest.fixture(params=OBJECTIVES, ids=[o[0] for o in OBJECTIVES])
def objective(request, oracle):
    name, hip, orc = request.param
    oracle.gicp_set_objective(orc)
    yield name, hip
    oracle.gicp_set_objective(0)


def _load(ctx, c):
    ctx.set_source(c.src)
    ctx.set_target(c.tgt)


def _ref(ctx, oracle, name):
    """the pairs, and both references' f and g at the case's states from the device's covariances: computed once (the
    context holds the case's clouds)"""
    if name not in _refs:
        c = GR.case(name)
        cs, ct = ctx.gicp_covariances()
        idx, _ = c.pairs()
        si = np.nonzero(idx >= 0)[0].astype(np.int32)
        ti = idx[si]
        M = GR.mahal_of_pairs(cs, ct, idx, c.T0f)
        vals = {"statistics": [], "pcl_sums": []}
        for x in c.states if len(si) else []:
            vals["pcl_sums"].append((oracle.gicp_fdf(c.src, c.tgt, si, ti, M, np.eye(4), x), GR.fdf_pcl(c.src, c.tgt, si, ti, M, x)))
            qf, qg, _ = oracle.gicp_fdf_statistics(c.src, c.tgt, si, ti, M, np.eye(4), c.T0f, x)
            vals["statistics"].append(((qf, qg), GR.fdf_statistics(c.src, c.tgt, si, ti, M, c.T0f, x)))
        _refs[name] = (idx, vals)
    return _refs[name]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _align(ctx, name, obj_name, hip):
    """the one-pair registration of a case (the context holds its clouds), kept for the batch to be compared with"""
    if (name, obj_name) not in _aligned:
        _aligned[(name, obj_name)] = ctx.gicp_align(objective=hip, max_corr=GR.case(name).max_corr)
    return _aligned[(name, obj_name)]


# ---------------------------------------------------------------------------------------------- a. one evaluation
@pytest.mark.parametrize("name", [n for n in GR.NAMES if n != "no_pair"])
def test_one_evaluation_matches_oracle_and_reference(wm, ctx, oracle, name):
    c = GR.case(name)
    _load(ctx, c)
    idx, vals = _ref(ctx, oracle, name)
    n_pairs = int((idx >= 0).sum())
    worst = {}
    failures = []
    for obj_name, hip, _ in OBJECTIVES:
        for k, x in enumerate(c.states):
            f, g, m = ctx.gicp_eval(c.T0f.astype(np.float64), x, objective=hip, max_corr=c.max_corr)
            gi, gd = ctx.correspondences()
            assert m == n_pairs and np.array_equal(gi, idx), (name, obj_name, k, m, n_pairs, np.nonzero(gi != idx)[0][:5])
            (of, og), (rf, rg) = vals[obj_name][k]
            b_f, b_g = GR.ref_vs_oracle(obj_name, c, k)
            d = dict(o_f=abs(f - of) / abs(of), o_g=_rel(g, og), r_f=abs(f - rf) / abs(rf), r_g=_rel(g, rg))
            for key, v in d.items():
                worst[(obj_name, key)] = max(worst.get((obj_name, key), 0.0), v)
            print("%s %s state %d: f %.17g (oracle %.17g)  " % (name, obj_name, k, f, of) + "  ".join("%s %.2e" % kv for kv in d.items()))
            # (every state's figures are printed before the first failure is raised)
            if not (np.isfinite(f) and np.isfinite(g).all() and d["o_f"] <= F_TOL and d["o_g"] <= G_TOL and
                    d["r_f"] <= max(F_TOL, 100 * b_f) and d["r_g"] <= max(G_TOL, 100 * b_g)):
                failures.append((obj_name, k, d))
    print("WORST %s (%d pairs): " % (name, n_pairs) + "  ".join("%s %s %.2e" % (o, key, v) for (o, key), v in sorted(worst.items())))
    assert not failures, failures


def test_no_pair_is_too_few_and_writes_no_nan(wm, ctx, oracle):
    c = GR.case("no_pair")
    _load(ctx, c)
    assert not (c.pairs()[0] >= 0).any()
    for obj_name, hip, orc in OBJECTIVES:
        p = wm.gicp_params(objective=hip, max_corr=c.max_corr)
        T = np.ascontiguousarray(c.T0f, np.float64)
        x = np.ascontiguousarray(c.states[1])
        f, m, g = C.c_double(7.0), C.c_int(-1), np.full(6, 7.0)
        dp = C.POINTER(C.c_double)
        rc = wm.lib().wm_gicp_eval(ctx._h, C.byref(p), T.ctypes.data_as(dp), x.ctypes.data_as(dp), C.byref(f),
                                   g.ctypes.data_as(dp), C.byref(m))
        assert rc == wm.WM_TOO_FEW and m.value == 0, (obj_name, rc, m.value)
        assert np.isfinite(f.value) and np.isfinite(g).all(), (obj_name, f.value, g)
        assert (ctx.correspondences()[0] == -1).all()
        got = ctx.gicp_align(objective=hip, max_corr=c.max_corr)
        oracle.gicp_set_objective(orc)
        try:
            want = oracle.gicp_align(*c.finite(), max_corr=c.max_corr)
        finally:
            oracle.gicp_set_objective(0)
        assert got["rc"] == wm.WM_TOO_FEW and got["T"] is None and not got["converged"] and not want["converged"]
        assert (got["n_corr"], got["iterations"], got["evaluations"]) == (0, 0, 0) == (want["n_corr"], want["iterations"], want["evaluations"])
        assert np.isfinite(got["f"])


# --------------------------------------------------------------------------------------- b. no knob changes a bit
@pytest.mark.parametrize("name", KNOB_CASES)
def test_no_knob_changes_a_bit(wm, ctx, oracle, name):
    """gicp_blocks caps the rows of partial sums an evaluation leaves for k_gicp_sum_fetch / k_gicp_quad_fetch -- and for
    the resident evaluator's last workgroup -- at min(ceil(n_src / 256), gicp_blocks).  What the cases reach (asserted by
    test_knob_cases_reach_the_row_counts_they_can): 1 and 2 rows everywhere, 1 to 5 on the nine sizes, 12 on the clouds
    of 3 000 points, and 13 and 14 on `lattice` (3 375 points, the largest cloud these tests allow) -- either side of the
    13 row groups of k_gicp_quad_fetch, whose group 0 makes its second trip at 14.  The 19 groups of gicp_sum_rows
    (247 slots of 13 components) take 20 rows to wrap, 5 121 points: NOT reached here -- the settings 19, 20 and 4096 are
    clamped to the cloud's own count and only have to change nothing.
    gicp_served: a launch per evaluation, the resident evaluator, its variant that keeps nothing on chip.  One answer."""
    c = GR.case(name)
    _load(ctx, c)
    idx, vals = _ref(ctx, oracle, name)
    evals, regs = {}, {}
    for nb in BLOCKS:
        ctx.set_option("gicp_blocks", nb)
        evals[nb] = [ctx.gicp_eval(c.T0f.astype(np.float64), x, objective=hip, max_corr=c.max_corr)
                     for _, hip, _ in OBJECTIVES for x in c.states]
        regs[(nb, "statistics")] = ctx.gicp_align(objective=wm.WM_GICP_OBJECTIVE_STATISTICS, max_corr=c.max_corr)
        for served in (0, 1, 2):
            ctx.set_option("gicp_served", served)
            regs[(nb, served)] = r = ctx.gicp_align(objective=wm.WM_GICP_OBJECTIVE_PCL_SUMS, max_corr=c.max_corr)
            if served == 0:
                assert r["served_evaluations"] == 0
            elif r["evaluations"] > 0:
                assert r["served_evaluations"] == r["evaluations"], (name, nb, served, r)
    # the first setting is the oracle's (agreeing on nothing does not pass) ...
    base = evals[BLOCKS[0]]
    want = [v[0] for obj_name, _, _ in OBJECTIVES for v in vals[obj_name]]
    for (f, g, m), (of, og) in zip(base, want):
        assert m == (idx >= 0).sum() and abs(f - of) <= F_TOL * abs(of) and _rel(g, og) <= G_TOL
    # ... and every other one is the first, bit for bit
    for nb in BLOCKS[1:]:
        for (f, g, m), (f0, g0, m0) in zip(evals[nb], base):
            assert m == m0 and f == f0 and np.array_equal(g, g0), (name, nb, f, f0)
    for key, r in regs.items():
        r0 = regs[(BLOCKS[0], "statistics" if key[1] == "statistics" else 0)]
        assert r["rc"] == r0["rc"] == 0, (name, key)
        assert (r["f"], r["evaluations"], r["iterations"], r["inner_total"], r["n_corr"]) == \
               (r0["f"], r0["evaluations"], r0["iterations"], r0["inner_total"], r0["n_corr"]), (name, key, r, r0)
        assert np.array_equal(r["T"], r0["T"]), (name, key)


def test_knob_cases_reach_the_row_counts_they_can():
    reached = {name: sorted({_rows(name, nb) for nb in BLOCKS}) for name in KNOB_CASES}
    assert reached["lattice"] == [1, 2, 13, 14] and reached["half"] == reached["utm"] == reached["dups"] == [1, 2, 12]
    assert [reached["n%d" % n][-1] for n in GR.SIZES] == [1, 1, 1, 1, 1, 1, 2, 3, 5]
    assert {13, 14} <= set().union(*reached.values()) and max(max(v) for v in reached.values()) == 14


# ---------------------------------------------------------------------------------------- c. whole registrations
@pytest.mark.parametrize("name", [n for n in GR.NAMES if n != "no_pair"])
def test_registrations_equal_the_oracles(wm, ctx, oracle, objective, name):
    obj_name, hip = objective
    c = GR.case(name)
    _load(ctx, c)
    got = _align(ctx, name, obj_name, hip)
    want = oracle.gicp_align(*c.finite(), max_corr=c.max_corr)
    keys = ("rc", "converged", "n_corr", "iterations", "inner_total", "evaluations", "f")
    print(name, obj_name, "device", {k: got[k] for k in keys}, "\n    oracle", {k: want[k] for k in keys})
    # PCL's align: an exception below four pairs, otherwise converged_ from the loop
    rc = wm.WM_OK if want["converged"] else (wm.WM_TOO_FEW if want["n_corr"] < 4 else wm.WM_NOT_CONVERGED)
    assert got["rc"] == rc and got["converged"] == want["converged"] and got["n_corr"] == want["n_corr"]
    assert (got["T"] is None) == (rc != wm.WM_OK)
    if name in ("one_pair", "three_pairs"):
        assert rc == wm.WM_TOO_FEW and got["iterations"] == 0 and got["evaluations"] == 0
    else:
        assert rc == wm.WM_OK  # (the oracle reports every other case converged -- four pairs too)
    if (name, obj_name) in LOOSE:
        dt, ang = pose_error(got["T"], want["T"])
        print("    (held to 1e-6: %.2e m, %.2e rad)" % (dt, ang))
        assert dt <= 1e-6 and ang <= 1e-6, (dt, ang)
        return
    assert (got["iterations"], got["inner_total"], got["evaluations"]) == (want["iterations"], want["inner_total"], want["evaluations"])
    assert got["f"] == want["f"]
    if rc == wm.WM_OK:
        assert np.array_equal(got["T"], want["T"]), np.abs(got["T"] - want["T"]).max()


# ------------------------------------------------------------------------------------------------- d. the batch
def _hold(failures, n, g, one, obj_name):
    try:
        if (n, obj_name) in LOOSE:
            assert g["rc"] == one["rc"] == 0
            dt, ang = pose_error(g["T"], one["T"])
            assert dt <= 1e-6 and ang <= 1e-6, (n, dt, ang)
        else:
            _same(g, one)
    except AssertionError as e:  # (every case is printed before the first failure is raised)
        failures.append((n, str(e)[:300]))


def test_batch_equals_the_one_pair_path(wm, ctx, objective):
    """every case through wm_gicp_batch_match against the one-pair path: one call for the cases that share max_corr = 5 m
    (it is a parameter of the call); `half` and `half_start` each in a call at THEIR max_corr, between two other pairs
    that are registered at that max_corr on the one-pair path too"""
    obj_name, hip = objective
    common = [n for n in GR.NAMES if GR.case(n).max_corr == GR.MAX_CORR]
    special = [n for n in GR.NAMES if n not in common]
    assert special == ["half", "half_start"]
    failures = []
    got = ctx.gicp_batch_match([(GR.case(n).src, GR.case(n).tgt) for n in common], objective=hip, max_corr=GR.MAX_CORR)
    for n, g in zip(common, got):
        if (n, obj_name) not in _aligned:
            _load(ctx, GR.case(n))
        print(n, obj_name, {k: g[k] for k in ("rc", "iterations", "evaluations", "n_corr", "f")})
        _hold(failures, n, g, _align(ctx, n, obj_name, hip), obj_name)
    for x in special:
        max_corr = GR.case(x).max_corr
        names = ["n65", x, "scene"]
        got = ctx.gicp_batch_match([(GR.case(n).src, GR.case(n).tgt) for n in names], objective=hip, max_corr=max_corr)
        for n, g in zip(names, got):
            print(n, "at the max_corr of", x, obj_name, {k: g[k] for k in ("rc", "iterations", "evaluations", "n_corr", "f")})
            _hold(failures, n, g, ctx.gicp_match(GR.case(n).src, GR.case(n).tgt, objective=hip, max_corr=max_corr), obj_name)
    assert not failures, failures


def test_first_search_holds_the_gate_on_both_paths(wm, ctx, objective):
    """half_start: under the identity, where wm_gicp_align and the batch make their first search, one source point is
    exactly max_corr from its neighbour -- not a pair.  One forced iteration reports that search's pairs."""
    obj_name, hip = objective
    c = GR.case("half_start")
    idx, _ = GR.pairs(c.src, c.tgt, np.eye(4), c.max_corr)
    _, d2 = GR.pairs(c.src, c.tgt, np.eye(4), 1e3)
    want = int((idx >= 0).sum())
    assert (d2.astype(np.float64) == c.max_corr * c.max_corr).sum() == 1 and (d2.astype(np.float64) <= c.max_corr * c.max_corr).sum() == want + 1
    one = ctx.gicp_match(c.src, c.tgt, objective=hip, max_corr=c.max_corr, force_iterations=1)
    n65, scene = GR.case("n65"), GR.case("scene")
    got = ctx.gicp_batch_match([(n65.src, n65.tgt), (c.src, c.tgt), (scene.src, scene.tgt)], objective=hip, max_corr=c.max_corr,
                               force_iterations=1)
    print(obj_name, "pairs of the first search: reference %d, one pair %d, batch %d" % (want, one["n_corr"], got[1]["n_corr"]))
    assert one["rc"] == got[1]["rc"] == 0 and one["iterations"] == got[1]["iterations"] == 1
    assert one["n_corr"] == want and got[1]["n_corr"] == want
    _same(got[1], one)
