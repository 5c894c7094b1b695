"""tests/sac_reference.py, the checker of wm_sac_segment, checked on the CPU: its two forms (one hypothesis at a time;
the stream in blocks) are equal on every case the GPU test uses, and the table of those cases is pinned -- the
max_iterations + 1 quirk, the adaptive bound stopping inside the third and the fourth block of 256, skipped entries
inside a long stream, the all-skipped exit.  Then the checker's own shapes: the strict threshold on dyadic layers, a
planted slab, the axis models."""
import math

import numpy as np
import pytest

import sac_reference as SR

SAME = ("status", "iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model", "axis_invalid")


# ------------------------------------------------------------------ the stream
def test_the_stream_is_the_contracts():
    assert SR.sm64(0) == 0 and SR.sm64(1) == 0x5692161D100B05E5  # (splitmix64's finaliser of 1)
    for n in (3, 4, 5, 64, 3000, 0x7FFFFFF0):
        blk = SR.samples_block(0, 0, 300, n)
        for j in (0, 1, 2, 17, 299):
            assert tuple(blk[j]) == SR.sample(0, j, n)
        assert (blk >= 0).all() and (blk < n).all()
        assert (blk[:, 0] != blk[:, 1]).all() and (blk[:, 0] != blk[:, 2]).all() and (blk[:, 1] != blk[:, 2]).all()
    # every triple of n = 3 is a permutation; a seed and an offset move the stream
    assert all(sorted(SR.sample(5, j, 3)) == [0, 1, 2] for j in range(50))
    assert tuple(SR.samples_block(9, 1000, 4, 777)[3]) == SR.sample(9, 1003, 777)
    assert SR.sample(0, 0, 3000) != SR.sample(1, 0, 3000)
    # the largest n: the indices reach the upper half
    assert SR.samples_block(0, 0, 300, 0x7FFFFFF0).max() > 0x40000000


def test_the_threshold_is_the_smallest_float_not_below():
    assert SR.thr_f(0.25) == np.float32(0.25)
    t = SR.thr_f(0.05)
    assert float(t) >= 0.05 and float(np.nextafter(t, np.float32(0))) < 0.05
    t = SR.thr_f(0.2)
    assert float(t) >= 0.2 and float(np.nextafter(t, np.float32(0))) < 0.2


# ------------------------------------------------------------------ the two forms
@pytest.mark.parametrize("i", range(len(SR.CASES)), ids=SR.case_id)
def test_the_two_forms_agree(i):
    name, thr, max_it, extra = SR.CASES[i]
    P = SR.shapes()[name]
    a = SR.run_literal(P, thr, max_it=max_it, **extra)
    for block in (256, 7):
        b = SR.run_blocks(P, thr, max_it=max_it, block=block, **extra)
        for k in SAME:
            assert a[k] == b[k], (k, a[k], b[k], block)
        if a["status"] == SR.OK:
            assert a["model_coefficients"].tobytes() == b["model_coefficients"].tobytes()
        else:
            assert a["model_coefficients"] is None and b["model_coefficients"] is None


# (shape, thr, max_it) -> iterations, skipped, best count, best entry   [the issue's table, seed 0]
TABLE = {
    ("exact_plane", 0.05, 50): (1, 0, 3000, 0),
    ("line", 0.05, 50): (0, 500, None, -1), ("line", 0.5, 1000): (0, 10000, None, -1),
    ("point", 0.05, 50): (0, 500, None, -1), ("point", 0.5, 1000): (0, 10000, None, -1),
    ("scene", 0.05, 50): (51, 0, 1256, 41), ("scene", 0.05, 1000): (61, 0, 1256, 41),
    ("scene", 0.5, 50): (24, 0, 1681, 2),
    ("holes", 0.05, 50): (51, 0, 1254, 41),
    ("lattice", 0.5, 1000): (658, 0, 645, 276),
    ("dups", 0.5, 1000): (919, 2, 513, 322),
    ("shell", 0.5, 1000): (1001, 0, 230, 891),
    ("clumps_outliers", 0.05, 50): (3, 0, 2986, 2),
}


def test_the_table():
    seen = set()
    for i, (name, thr, max_it, extra) in enumerate(SR.CASES):
        if extra or (name, thr, max_it) not in TABLE:
            continue
        seen.add((name, thr, max_it))
        it, skipped, best, entry = TABLE[(name, thr, max_it)]
        o = SR.case(i)
        assert (o["iterations"], o["skipped"], o["best_hypothesis"]) == (it, skipped, entry), (name, thr, max_it, o)
        assert o["hypotheses"] == it + skipped
        if best is None:
            assert o["status"] == SR.NOT_CONVERGED and o["coefficients"] is None and len(o["indices"]) == 0
        else:
            assert o["status"] == SR.OK and o["n_inliers_model"] == best
    assert seen == set(TABLE)
    # what the rows are there for
    assert TABLE[("scene", 0.05, 50)][0] == 50 + 1 and TABLE[("shell", 0.5, 1000)][0] == 1000 + 1  # the quirk
    assert 2 * 256 < TABLE[("lattice", 0.5, 1000)][0] < 3 * 256 < TABLE[("dups", 0.5, 1000)][0] + 2 < 4 * 256


def test_selection_and_refit_of_every_case():
    for i, (name, thr, max_it, extra) in enumerate(SR.CASES):
        P = SR.shapes()[name]
        o, raw = SR.case(i), SR.case(i, optimize=False)
        if o["status"] != SR.OK:
            continue
        th = SR.thr_f(thr)
        assert raw["refined"] == 0 and raw["coefficients"].tobytes() == raw["model_coefficients"].tobytes()
        assert len(raw["indices"]) == raw["n_inliers_model"]  # without a refit the selection IS the model's count
        for r in (o, raw):
            idx, lab = r["indices"], r["labels"]
            assert (np.diff(idx) > 0).all() and (lab[idx] == SR.INLIER).all() and (lab == SR.INLIER).sum() == len(idx)
            assert ((lab == SR.NONE) == ~np.isfinite(P).all(1)).all()
            c = r["coefficients"].astype(np.float64)
            d = np.abs(P[idx].astype(np.float64) @ c[:3] + c[3])
            assert (d < float(th) * (1 + 1e-5) + 1e-6 * max(1.0, abs(c[3]))).all()
        assert o["refined"] == 1
        f = SR.refit(P, o["model_coefficients"], thr)
        n = o["coefficients"][:3].astype(np.float64)
        assert n @ o["model_coefficients"][:3].astype(np.float64) > 0
        assert abs(np.linalg.norm(n) - 1) <= 4 * 2.0 ** -23
        assert n @ f["C"] @ n <= f["lam"][0] * (1 + 1e-9) + 1e-12 * f["lam"][2]


# ------------------------------------------------------------------ the checker's own shapes
def test_decks_the_threshold_is_strict():
    P = SR.shapes()["decks"]
    z = P[:, 2]
    assert len(P) == 1792 and ((z == 0).sum(), (z == 0.25).sum(), (z == -0.5).sum()) == (1024, 512, 256)
    flat = np.array([0, 0, 1, 0], np.float32)
    m = SR.inliers(P, flat, SR.thr_f(0.25))
    assert m.sum() == 1024 and (z[m] == 0).all()  # 0.25 is not < 0.25: the z = 0 plane takes its own layer only
    assert SR.inliers(P, flat, np.nextafter(np.float32(0.25), np.float32(1))).sum() == 1024 + 512
    # what the checker finds: a tilted plane through two layers beats every single layer
    o = SR.case([c[0] for c in SR.CASES].index("decks"))
    assert (o["iterations"], o["skipped"], o["best_hypothesis"], o["n_inliers_model"]) == (7, 0, 6, 1450)
    assert set(np.unique(z[SR.inliers(P, o["model_coefficients"], SR.thr_f(0.25))])) == {0.0, 0.25}


def test_the_planted_slab_is_recovered():
    i = [c[0] for c in SR.CASES].index("slab")
    o = SR.case(i)
    want = SR.SLAB_NORMAL / np.linalg.norm(SR.SLAB_NORMAL)
    for c in (o["model_coefficients"], o["coefficients"]):
        n = c[:3].astype(np.float64)
        ang = math.degrees(math.acos(min(1.0, abs(n @ want) / np.linalg.norm(n))))
        assert ang < 1.0, ang
    assert o["n_inliers_model"] >= 1800 and len(o["indices"]) >= 1900


def test_axis_models_on_the_scene():
    ids = [SR.case_id(i) for i in range(len(SR.CASES))]
    plain = SR.case(ids.index("scene-0.05-50"))
    perp = SR.case(ids.index("scene-0.05-50-model1"))
    # perpendicular to z, eps 0.1: the floor -- here the very model of the plain run, with entries refused on the way
    assert perp["axis_invalid"] == 23 and perp["iterations"] == 51
    assert perp["model_coefficients"].tobytes() == plain["model_coefficients"].tobytes()
    assert abs(perp["coefficients"][2]) > math.cos(0.1)
    # parallel to z: most entries are refused.  Entry 0 is: its count of 0 sets k as in PCL, the loop goes on, and no
    # refused entry is ever the model -- 51 refusals leave no model, 201 entries hold three walls' worth of samples
    par50 = SR.case(ids.index("scene-0.05-50-model2"))
    assert (par50["status"], par50["iterations"], par50["axis_invalid"], par50["best_hypothesis"]) == (SR.NOT_CONVERGED, 51, 51, -1)
    par = SR.case(ids.index("scene-0.05-200-model2"))
    assert (par["status"], par["iterations"], par["axis_invalid"]) == (SR.OK, 201, 198)
    assert (par["best_hypothesis"], par["n_inliers_model"]) == (110, 60)
    assert abs(par["model_coefficients"][2]) < math.sin(0.1) and abs(par["coefficients"][0]) > 0.99  # the wall at x = -50
    a, ce, se = SR.axis_consts((0, 0, 2.5), 0.1)
    assert a.tolist() == [0, 0, 1] and ce == np.float32(math.cos(0.1)) and se == np.float32(math.sin(0.1))


def test_small_clouds_have_no_model():
    for n in (0, 1, 2):
        o = SR.segment(np.zeros((n, 3), np.float32), 0.1)
        assert o["status"] == SR.NOT_CONVERGED and o["hypotheses"] == 0 and o["best_hypothesis"] == -1
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    o = SR.segment(tri, 0.1)
    assert o["status"] == SR.OK and o["n_inliers_model"] == 3 and o["refined"] == 0 and o["iterations"] == 1
    o = SR.segment(np.full((64, 3), np.nan, np.float32), 0.1, max_it=5)
    assert o["status"] == SR.NOT_CONVERGED and o["skipped"] == 50 and o["iterations"] == 0
