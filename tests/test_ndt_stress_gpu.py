"""NDT on stress shapes (tests/ndt_reference.py): the voxel model and k_ndt_derivs against the oracle AND against a plain
numpy reference on collapsed axes, threshold voxels, points on voxel faces, crowded voxels, non-finite rows, lattices of
more than 2^32 cells, and clouds 600 to 1000 km from the origin -- where absolute voxel coordinates no longer fit the 21
bits per axis of a voxel key, and keys are therefore formed relative to the lattice's low corner.

At those offsets a float has 16 positions per voxel axis, so the far shapes are a dyadic lattice whose voxel statistics
are exact in double (tests/test_ndt_reference_cpu.py: the model is the centred model shifted, bit for bit).  Three anchors
hold there: the derivatives at translation-only poses (a rotation throws every point out of the lattice), the equality of
the device's own look-ups, and the batch against the one-pair path.  Whole registrations are compared with the oracle near
the origin only: the Hessian's rotational entries are 1e11 times its translational ones out there, and iteration counts
are not stable to the last bits.

Tolerances: test_ndt_gpu.py's -- 1e-9 on the score, 1e-8 of the largest entry on gradient and Hessian (the gradient's
is the larger of that and 100 times the reference's own distance from the oracle, NR.REF_VS_ORACLE_GRAD: the margin for
the device's summation order and its exp).  Worst differences measured on an MI355X over every shape and pose (this file
prints them with -s), relative as above:
    GPU against oracle:           score 7.1e-15, gradient 2.8e-12, Hessian 3.7e-11 (both on outliers64's rotated pose;
                                  1.7e-13 and 8.4e-14 on every other shape)
    GPU against numpy reference:  score 5.2e-12 (`line`), gradient 1.6e-11 (outliers64; 2.7e-13 elsewhere bar `line`'s 7e-12)
    far shapes, translation block on its own: gradient 2.1e-15 / 6.1e-15 (oracle / reference), Hessian 1.7e-15"""
import os

import numpy as np
import pytest

import ndt_reference as NR
from helpers import TOL_R, TOL_T, pose_error
from test_ndt_batch_gpu import _close

pytestmark = pytest.mark.gpu

GRAD_TOL = max(1e-8, 100 * NR.REF_VS_ORACLE_GRAD)
REG = dict(step_size=0.1, t_eps=1e-6, max_iter=35)  # the registrations' parameters (res: the shape's)
_refs = {}


def _ref(oracle, name):
    """the oracle's grid, the numpy model and both references' derivatives at the shape's poses: computed once"""
    if name not in _refs:
        s = NR.shape(name)
        grid = oracle.NdtGrid(s.tgt, s.res)
        mdl = NR.model(s.tgt, s.res)
        finite = s.src[np.isfinite(s.src).all(1)]
        prm = oracle.ndt_params(res=s.res)
        _refs[name] = (grid, [(pose, grid.derivatives(finite, pose, prm), NR.score_gradient(s.src, pose, mdl, s.res))
                              for pose in s.poses])
    return _refs[name]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _context(wm, dense=None):
    if dense is None:
        return wm.Context(0)
    os.environ["WM_TUNE_NDT_DENSE"] = str(dense)  # read when a context is created
    try:
        return wm.Context(0)
    finally:
        del os.environ["WM_TUNE_NDT_DENSE"]


def _same_derivs(a, b, what):
    (s1, g1, H1, n1), (s0, g0, H0, n0) = a, b
    assert n1 == n0 and s1 == s0 and np.array_equal(g1, g0) and np.array_equal(H1, H0), (what, s1, s0)


def _same_align(a, b, what):
    assert a["rc"] == b["rc"] == 0 and np.array_equal(a["T"], b["T"]), what
    assert (a["iterations"], a["evaluations"], a["n_voxels"]) == (b["iterations"], b["evaluations"], b["n_voxels"]), what


# ------------------------------------------------------------------------------------------------ a. derivatives
@pytest.mark.parametrize("name", [n for n in NR.NAMES if n != "too_wide"])
def test_derivatives_match_oracle_and_reference(wm, ctx, oracle, name):
    s = NR.shape(name)
    grid, refs = _ref(oracle, name)
    ctx.set_source(s.src)
    ctx.set_target(s.tgt)
    worst = dict(o_s=0.0, o_g=0.0, o_H=0.0, r_s=0.0, r_g=0.0, o_gt=0.0, o_Ht=0.0, r_gt=0.0)
    failures = []
    for pose, (os_, og, oH), (rs, rg) in refs:
        sc, g, H, nv = ctx.ndt_derivatives(pose, res=s.res)
        assert nv == grid.size(), (name, nv, grid.size())
        assert os_ != 0.0 and np.isfinite(sc) and np.isfinite(g).all() and np.isfinite(H).all()
        d = dict(o_s=abs(sc - os_) / abs(os_), o_g=_rel(g, og), o_H=_rel(H, oH), r_s=abs(sc - rs) / abs(rs), r_g=_rel(g, rg))
        if s.far:  # the translation block relative to ITS largest entry: the rotational entries are 1e5 times larger
            d.update(o_gt=_rel(g[:3], og[:3]), o_Ht=_rel(H[:3, :3], oH[:3, :3]), r_gt=_rel(g[:3], rg[:3]))
        for k, v in d.items():
            worst[k] = max(worst[k], v)
        print("%s %s: score %.17g (oracle %.17g)  " % (name, pose.tolist(), sc, os_) + "  ".join("%s %.2e" % kv for kv in d.items()))
        try:
            assert abs(sc - os_) <= 1e-9 * abs(os_) and abs(sc - rs) <= 1e-9 * abs(rs)
            np.testing.assert_allclose(g, og, rtol=GRAD_TOL, atol=GRAD_TOL * np.abs(og).max())
            np.testing.assert_allclose(g, rg, rtol=GRAD_TOL, atol=GRAD_TOL * np.abs(rg).max())
            np.testing.assert_allclose(H, oH, rtol=1e-8, atol=1e-8 * np.abs(oH).max())
            if s.far:
                np.testing.assert_allclose(g[:3], og[:3], rtol=GRAD_TOL, atol=GRAD_TOL * np.abs(og[:3]).max())
                np.testing.assert_allclose(g[:3], rg[:3], rtol=GRAD_TOL, atol=GRAD_TOL * np.abs(rg[:3]).max())
                np.testing.assert_allclose(H[:3, :3], oH[:3, :3], rtol=1e-8, atol=1e-8 * np.abs(oH[:3, :3]).max())
        except AssertionError as e:  # (every pose's figures are printed before the first failure is raised)
            failures.append((pose.tolist(), str(e)[:400]))
    print("WORST %s: " % name + "  ".join("%s %.2e" % kv for kv in worst.items()))
    assert not failures, failures


# ------------------------------------------------------------------------- b. one answer from every look-up
@pytest.mark.parametrize("name", ["lattice", "utm", "utm_edge", "outliers64"])
def test_every_lookup_and_key_width_gives_the_same_bits(wm, oracle, name):
    """float4 cells, the dense table and the hash grid (WM_TUNE_NDT_DENSE 2, 1, 0), the points sorted by 32- or by 64-bit
    keys: the same voxels in the same neighbour order, so every accumulated double is the same -- and the oracle's, so
    that agreeing on nothing does not pass.  (outliers64 takes 64-bit keys and the hash grid whatever is asked.)"""
    s = NR.shape(name)
    grid, refs = _ref(oracle, name)
    out = {}
    for dense in (2, 1, 0):
        c = _context(wm, dense)
        c.set_source(s.src)
        c.set_target(s.tgt)
        for keys64 in (0, 1):
            c.set_option("ndt_keys64", keys64)
            derivs = [c.ndt_derivatives(pose, res=s.res) for pose in s.poses]
            align = None
            if name == "lattice":
                c.set_source(s.extra["moved"])
                align = c.ndt_align(res=s.res, **REG)
                c.set_source(s.src)
            out[(dense, keys64)] = (derivs, align)
        c.close()
    base_d, base_a = out[(1, 0)]
    for (pose, (os_, og, oH), _), (sc, g, H, nv) in zip(refs, base_d):
        assert nv == grid.size() and os_ != 0.0 and abs(sc - os_) <= 1e-9 * abs(os_), (name, pose, sc, os_)
    for key, (derivs, align) in out.items():
        for a, b in zip(derivs, base_d):
            _same_derivs(a, b, (name, key))
        if align is not None:
            _same_align(align, base_a, (name, key))


# --------------------------------------------------------------------------------------------------- c. the batch
def test_batch_equals_the_one_pair_path_near_and_far(wm, ctx):
    """wm_ndt_small.hip indexes its table from the lattice's corner; the one-pair path must see the same voxels"""
    names = ["lattice", "utm", "utm_neg", "slab"]
    pairs = [(NR.shape(n).extra["moved"], NR.shape(n).tgt) for n in names]
    got = ctx.ndt_batch_match(pairs, res=0.5, **REG)
    for n, (src, tgt), g in zip(names, pairs, got):
        ctx.set_source(src)
        ctx.set_target(tgt)
        one = ctx.ndt_align(res=0.5, **REG)
        print("%s: batch %s\n    one pair %s" % (n, {k: g[k] for k in ("rc", "converged", "iterations", "n_voxels", "score")},
                                                  {k: one[k] for k in ("rc", "converged", "iterations", "n_voxels", "score")}))
        assert one["n_voxels"] == 1767 if n != "slab" else one["n_voxels"] > 700
        if NR.shape(n).far:  # iteration counts are not stable to the last bits out there (see the top of this file)
            assert (g["rc"], g["converged"], g["n_voxels"]) == (one["rc"], one["converged"], one["n_voxels"]), n
            # ... but both registrations took place: a path that finds no voxel "converges" at once, on a score of 0,
            # with the same three values
            assert g["iterations"] > 0 and one["iterations"] > 0 and g["score"] > 0.1 and one["score"] > 0.1, n
        else:
            _close(g, one)


# ------------------------------------------------------------------------ d. registrations near the origin
@pytest.mark.parametrize("name", ["lattice", "slab", "crowded", "faces", "faces_03"])
def test_registrations_match_the_oracle(wm, ctx, oracle, name):
    s = NR.shape(name)
    ctx.set_source(s.extra["moved"])
    ctx.set_target(s.tgt)
    got = ctx.ndt_align(res=s.res, **REG)
    want = oracle.ndt_align(s.extra["moved"], s.tgt, res=s.res, **REG)
    print(name, {k: got[k] for k in ("rc", "converged", "iterations", "n_voxels")}, want["iterations"], want["n_voxels"])
    assert got["rc"] == want["rc"] == 0 and got["converged"] and want["converged"]
    assert got["n_voxels"] == want["n_voxels"] and got["iterations"] == want["iterations"]
    dt, ang = pose_error(got["T"], want["T"])
    assert dt <= TOL_T and ang <= TOL_R, (dt, ang)
    if name == "lattice":  # the shift comes back
        assert want["iterations"] == 7 and np.linalg.norm(got["T"][:3, 3] - np.array(NR.SHIFT)) < 0.01


# --------------------------------------------------------------------------------------------------- e. edges
def test_nothing_to_match_gives_the_oracles_answer(wm, ctx, oracle):
    s = NR.shape("threshold")
    nan_src = np.full((7, 3), np.nan, np.float32)  # a source of which no point is left
    one = s.tgt[12:13] + np.float32(0.01)  # inside a valid voxel of 7 points: a Hessian of rank 3
    for what, src, tgt in (("no valid voxel", s.src, s.extra["tgt_none"]), ("one point", one, s.tgt),
                           ("one point, no voxel near", s.tgt[:1], s.tgt), ("no finite point", nan_src, s.tgt)):
        ctx.set_source(src)
        ctx.set_target(tgt)
        got = ctx.ndt_align(res=s.res)
        want = oracle.ndt_align(src[np.isfinite(src).all(1)], tgt, res=s.res)
        print(what, {k: got[k] for k in ("rc", "converged", "iterations", "n_voxels")}, want["iterations"])
        assert (got["rc"], got["converged"], got["n_voxels"]) == (want["rc"], want["converged"], want["n_voxels"]), (what, got, want)
        assert got["T"] is not None and np.isfinite(got["T"]).all(), what
        if what != "one point":  # nothing to step along: the identity
            assert got["iterations"] == want["iterations"] == 0 and np.array_equal(got["T"], want["T"]), what
        sc, g, H, nv = ctx.ndt_derivatives(np.zeros(6), res=s.res)
        assert nv == want["n_voxels"] and np.isfinite([sc]).all() and np.isfinite(g).all() and np.isfinite(H).all(), what
    with pytest.raises(wm.WmError):  # an EMPTY cloud is refused (WM_ERR_STATE), as in a batch: test_ndt_batch_gpu.py
        ctx.set_source(np.zeros((0, 3), np.float32))
        ctx.ndt_align(res=s.res)


def _lattice_bytes(c):
    s = NR.shape("lattice")
    c.set_source(s.src)
    c.set_target(s.tgt)
    derivs = [c.ndt_derivatives(pose, res=s.res) for pose in s.poses]
    c.set_source(s.extra["moved"])
    return derivs, c.ndt_align(res=s.res, **REG)


def test_a_refused_or_a_far_target_leaves_nothing_behind(wm, ctx):
    fresh = wm.Context(0)
    want_d, want_a = _lattice_bytes(fresh)
    fresh.close()
    assert want_a["rc"] == 0 and want_a["n_voxels"] == 1767
    # a target that spans more than 2^20 voxels is refused with a message ...
    w = NR.shape("too_wide")
    ctx.set_source(w.src)
    ctx.set_target(w.tgt)
    for call in (lambda: ctx.ndt_derivatives(np.zeros(6), res=w.res), lambda: ctx.ndt_align(res=w.res)):
        with pytest.raises(wm.WmError) as e:
            call()
        assert "2^20 voxels" in str(e.value) and wm.lib().wm_strerror(wm.WM_ERR_ARG).decode() in str(e.value)
    # ... and the context registers the next pair as a fresh one does
    got_d, got_a = _lattice_bytes(ctx)
    for a, b in zip(got_d, want_d):
        _same_derivs(a, b, "after too_wide")
    _same_align(got_a, want_a, "after too_wide")
    # a model 700 km out, then one at the origin (and the other way round: the far one is the oracle's still)
    u = NR.shape("utm")
    ctx.set_source(u.src)
    ctx.set_target(u.tgt)
    far = [ctx.ndt_derivatives(pose, res=u.res) for pose in u.poses]
    assert far[0][3] == 1767 and far[0][0] != 0.0
    got_d, got_a = _lattice_bytes(ctx)
    for a, b in zip(got_d, want_d):
        _same_derivs(a, b, "after utm")
    _same_align(got_a, want_a, "after utm")
    ctx.set_source(u.src)
    ctx.set_target(u.tgt)
    for a, b in zip([ctx.ndt_derivatives(pose, res=u.res) for pose in u.poses], far):
        _same_derivs(a, b, "utm again")


def test_crowded_model_does_not_depend_on_who_forms_a_voxels_sums(wm, ctx, oracle):
    """voxels of 31, 32, 33 and 127, 128, 129 points: a lane's or a wave's at the default split of this grid (32), at the
    one of large grids (128), with every voxel a wave's (0) and every voxel a lane's (1 << 30) -- one model"""
    s = NR.shape("crowded")
    grid, refs = _ref(oracle, "crowded")
    out = []
    for split in (-1, 0, 32, 128, 1 << 30):
        ctx.set_option("ndt_vox_split", split)
        ctx.set_source(s.src)
        ctx.set_target(s.tgt)
        derivs = [ctx.ndt_derivatives(pose, res=s.res) for pose in s.poses]
        ctx.set_source(s.extra["moved"])
        out.append((split, derivs, ctx.ndt_align(res=s.res, **REG)))
    ctx.set_option("ndt_vox_split", -1)
    _, d0, a0 = out[0]
    assert d0[0][3] == grid.size() == 135 and abs(d0[0][0] - refs[0][1][0]) <= 1e-9 * abs(refs[0][1][0])
    for split, d, a in out[1:]:
        for x, y in zip(d, d0):
            _same_derivs(x, y, split)
        _same_align(a, a0, split)
