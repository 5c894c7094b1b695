"""The checker of the NDT stress tests, checked: tests/ndt_reference.py's numpy statement of the voxel model and of the
score and gradient against the C oracle (oracle/ndt.c) on every stress shape -- two independent statements (centred data
and LAPACK's eigh against PCL's raw sums and a Jacobi iteration; a Jacobian from rotation matrices against PCL's table
of vectors) that must agree on every voxel's validity and to rounding on everything else -- and the generators held to
what they claim, so that the device tests reach the mechanisms they name."""
import numpy as np
import pytest

import ndt_reference as NR


def _oracle_model(oracle, s, tgt=None):
    grid = oracle.NdtGrid(s.tgt if tgt is None else tgt, s.res)
    ijk, mean, icov, cnt = grid.export()
    return grid, {tuple(int(v) for v in c): (int(n), m, ic) for c, m, ic, n in zip(ijk, mean, icov, cnt)}


@pytest.fixture(scope="module")
def worst():
    w = {"icov": 0.0, "score": 0.0, "grad": 0.0}
    yield w
    print("\nworst numpy reference against oracle: icov %.3g  score %.3g  gradient %.3g" % (w["icov"], w["score"], w["grad"]))


@pytest.mark.parametrize("name", NR.NAMES)
def test_model_equals_the_oracles(oracle, worst, name):
    s = NR.shape(name)
    grid, om = _oracle_model(oracle, s)
    nm = NR.model(s.tgt, s.res)
    valid = {c for c, v in nm.items() if v[4]}
    assert valid == set(om), (name, sorted(valid ^ set(om))[:5])  # not ONE voxel on which PCL's rule depends on the solver
    assert grid.size() == len(valid)
    w_icov = 0.0
    for c in valid:
        n, mean, cov, icov, _ = nm[c]
        on, omean, oicov = om[c]
        assert n == on
        # (relative to the voxel: its largest coordinate or, next to the origin, its size)
        assert np.abs(mean - omean).max() <= 1e-12 * max(np.abs(mean).max(), s.res), (name, c)
        w_icov = max(w_icov, np.abs(icov - oicov).max() / np.abs(icov).max())
    print("%s: %d voxels, %d valid, icov worst %.3g" % (name, len(nm), len(valid), w_icov))
    worst["icov"] = max(worst["icov"], w_icov)
    assert w_icov <= NR.REF_VS_ORACLE_ICOV, (name, w_icov)


@pytest.mark.parametrize("name", NR.NAMES)
def test_score_and_gradient_equal_the_oracles(oracle, worst, name):
    s = NR.shape(name)
    grid = oracle.NdtGrid(s.tgt, s.res)
    nm = NR.model(s.tgt, s.res)
    finite = s.src[np.isfinite(s.src).all(1)]
    for pose in s.poses:
        sc, g = NR.score_gradient(s.src, pose, nm, s.res)
        osc, og, _ = grid.derivatives(finite, pose, oracle.ndt_params(res=s.res))
        assert osc != 0.0, (name, pose)  # the shape's source meets its target at every pose
        e_s = abs(sc - osc) / abs(osc)
        e_g = np.abs(g - og).max() / np.abs(og).max()
        if s.far:  # the rotational entries are 1e5 times the others: the translation block on its own as well
            e_g = max(e_g, np.abs(g[:3] - og[:3]).max() / np.abs(og[:3]).max())
        print("%s %s: score %.17g (%.3g)  gradient %.3g" % (name, pose.tolist(), osc, e_s, e_g))
        worst["score"], worst["grad"] = max(worst["score"], e_s), max(worst["grad"], e_g)
        assert e_s <= NR.REF_VS_ORACLE_SCORE and e_g <= NR.REF_VS_ORACLE_GRAD, (name, pose, e_s, e_g)


@pytest.mark.parametrize("name", ["utm", "utm_neg", "utm_edge"])
def test_a_far_lattice_is_the_lattice_shifted(oracle, name):
    """means exactly, inverse covariances bit for bit, the same voxels valid: by the reference and by the oracle"""
    s, base = NR.shape(name), NR.shape("lattice")
    D = s.extra["offset"]
    dc = tuple(int(v) for v in D / s.res)
    assert np.array_equal(np.array(dc) * s.res, D)
    c = NR.cells_of(s.tgt, s.res)
    assert np.abs(c).max() >= 1 << 20
    if name == "utm_edge":
        assert c[:, 0].min() < (1 << 20) <= c[:, 0].max() and c[:, 1].min() < -(1 << 20) <= c[:, 1].max()
    _, om_far = _oracle_model(oracle, s)
    _, om_base = _oracle_model(oracle, base)
    nm_far, nm_base = NR.model(s.tgt, s.res), NR.model(base.tgt, base.res)
    assert len(om_base) == len(om_far) == len(nm_base) > 1500 and all(v[0] == 8 and v[4] for v in nm_base.values())
    for cell, (n, mean, icov) in om_base.items():
        far = om_far[tuple(a + b for a, b in zip(cell, dc))]
        assert far[0] == n and np.array_equal(far[1], mean + D) and np.array_equal(far[2], icov), cell
    for cell, (n, mean, cov, icov, valid) in nm_base.items():
        far = nm_far[tuple(a + b for a, b in zip(cell, dc))]
        assert far[0] == n and far[4] == valid and np.array_equal(far[1], mean + D) and np.array_equal(far[3], icov), cell


def test_lattice_sizes_are_on_the_stated_side_of_the_rules():
    s = NR.shape("outliers64")
    dims = NR.lattice_dims(s.tgt, s.res)
    assert max(dims) <= 1 << 20 and dims[0] * dims[1] * dims[2] > 1 << 32  # 64-bit sort keys, and far beyond a dense table
    assert (dims[0] + 4) * (dims[1] + 4) * (dims[2] + 4) > 32 << 20
    w = NR.shape("too_wide")
    assert max(NR.lattice_dims(w.tgt, w.res)) > 1 << 20
    assert np.array_equal(w.tgt[:len(s.tgt)], s.tgt)
    assert NR.lattice_dims(NR.shape("plane_exact").tgt, 0.5)[2] == 1
    for name in NR.NAMES:  # the dense table and the float4 cells are what every other shape's look-ups go through
        if name not in ("outliers64", "too_wide"):
            d = NR.lattice_dims(NR.shape(name).tgt, NR.shape(name).res)
            assert (d[0] + 4) * (d[1] + 4) * (d[2] + 4) <= 4 << 20, name


def test_far_clumps_of_outliers64_are_valid_voxels():
    s = NR.shape("outliers64")
    nm = NR.model(s.tgt, s.res)
    far = [v for c, v in nm.items() if abs(c[0]) >= 400000 - 1]
    assert len(far) == 2 and all(v[0] == 8 and v[4] for v in far)
    assert sum(1 for v in nm.values() if v[4]) > 100


def test_eigenvalue_branches_are_reached_unambiguously():
    """slab: one eigenvalue raised; line: two; plane_exact: one, from exactly zero.  No raised eigenvalue is rounding
    noise -- the raw sums of these clouds (|p| <= 20, a few dozen points) are good to 1e-13 -- except plane_exact's,
    which is an exact zero in every solver; in voxels of ten points and more the raised ones are far below the bar."""
    for name, raised in (("slab", 1), ("line", 2), ("plane_exact", 1)):
        s = NR.shape(name)
        n_valid = 0
        for c, (n, mean, cov, icov, valid) in NR.model(s.tgt, s.res).items():
            if n < NR.MIN_POINTS:
                continue
            p = s.tgt[(NR.cells_of(s.tgt, s.res) == c).all(1)].astype(np.float64)
            w = np.linalg.eigvalsh(np.cov(p.T, bias=True))
            assert valid and w[2] > 0, (name, c)
            n_valid += 1
            if name == "plane_exact":
                assert w[0] == 0.0 or abs(w[0]) < 1e-30
            else:
                assert (w[:raised] > 1e-10).all(), (name, c, w)
            if n >= 10:  # (a voxel of six to nine points may be anything: it only has to be unambiguous, above)
                assert (w[:raised] < 1e-3 * w[2]).all() and (w[raised:] > 0.0).all(), (name, c, w)
        assert n_valid >= 100, name


def test_threshold_voxels():
    s = NR.shape("threshold")
    nm = NR.model(s.tgt, s.res)
    by_count = {}
    for c, v in nm.items():
        by_count.setdefault(v[0], []).append(v[4])
    assert by_count[5] == [False] * 4 and by_count[7] == [True] * 4
    assert sorted(by_count[6]) == [False] + [True] * 4  # the six coincident points: a covariance of exactly zero
    six = nm[(8, 0, 0)]
    assert six[0] == 6 and not six[4] and np.array_equal(six[1], [4.25, 0.25, 0.25])
    none = NR.model(s.extra["tgt_none"], s.res)
    assert len(none) == 12 and max(v[0] for v in none.values()) == 5 and not any(v[4] for v in none.values())


def test_faces_and_crowded_and_holes_hold_what_they_name():
    for name in ("faces", "faces_03"):
        s = NR.shape(name)
        for cloud in (s.tgt, s.src):
            k = np.rint(cloud.astype(np.float64) / s.res)
            on = cloud == (k * s.res).astype(np.float32)  # exactly on a face
            cell = NR.cells_of(cloud, s.res)
            assert on.sum() > 500 and (cloud < 0).any() and np.signbit(cloud[cloud == 0]).any()
            assert (cell[on] == k[on]).any()
            if name == "faces_03":  # the float product decides: some land a cell below their face
                assert (cell[on] == k[on] - 1).any() and np.isin(cell[on] - k[on], (-1, 0)).all()
            else:
                assert (cell[on] == k[on]).all()
    s = NR.shape("crowded")
    counts = sorted(v[0] for v in NR.model(s.tgt, s.res).values())
    assert counts == s.extra["counts"] and counts[-7:] == [31, 32, 33, 127, 128, 129, 5000]
    assert len(s.tgt) <= 192 * len(counts) and len(counts) <= 32768  # lanes and waves split the voxels, at 32 points
    big = np.nonzero((NR.cells_of(s.tgt, s.res) == 0).all(1))[0]
    assert len(big) == 5000 and np.ptp(big) > 6000
    s = NR.shape("holes")
    for cloud in (s.tgt, s.src):
        bad = ~np.isfinite(cloud)
        assert all(bad[:, a].any() for a in range(3)) and np.isnan(cloud).any() and np.isposinf(cloud).any() and np.isneginf(cloud).any()
    assert (np.abs(s.src[np.isfinite(s.src).all(1)]) == 1e9).any(1).sum() >= 12


def test_reference_on_a_case_small_enough_to_read():
    # eight corners of a cube of side 0.25 in the voxel at the origin, res 0.5: mean at its centre, covariance
    # (side / 2)^2 (n - 1) / n on the diagonal
    cube = np.float32([[x, y, z] for x in (0.125, 0.375) for y in (0.125, 0.375) for z in (0.125, 0.375)])
    m = NR.model(np.r_[cube, np.float32([[np.nan, 0, 0], [0.7, 0.1, 0.1]])], 0.5)
    assert sorted(m) == [(0, 0, 0), (1, 0, 0)] and m[(1, 0, 0)][0] == 1 and not m[(1, 0, 0)][4]
    n, mean, cov, icov, valid = m[(0, 0, 0)]
    assert n == 8 and valid and np.array_equal(mean, [0.25] * 3)
    np.testing.assert_allclose(cov, np.eye(3) * 0.125 ** 2 * 7 / 8, rtol=0, atol=1e-17)
    np.testing.assert_allclose(icov, np.eye(3) / (0.125 ** 2 * 7 / 8), rtol=1e-15, atol=1e-12)
    # one point at the mean: x' - mean = 0, so the score is -d1 and the gradient zero; moved by t along x, the
    # gradient is d1 d2 exp(-d2 q / 2) t / var along x and zero elsewhere -- and its rotational part J^T of that
    d1, d2 = NR.gauss_constants(0.5)
    sc, g = NR.score_gradient(np.float32([[0.25, 0.25, 0.25]]), np.zeros(6), m, 0.5)
    assert sc == -d1 and not g.any()
    var, t = 0.125 ** 2 * 7 / 8, 0.0625
    sc, g = NR.score_gradient(np.float32([[0.25, 0.25, 0.25]]), np.array([t, 0, 0, 0, 0, 0]), m, 0.5)
    e = np.exp(-d2 * t * t / var / 2)
    gx = d1 * d2 * e * t / var
    assert abs(sc + d1 * e) <= 1e-15 * abs(sc)
    # d(Rx Ry Rz x)/d(angles) at zero angles: columns (0, -z, y), (z, 0, -x), (-y, x, 0); their x components 0, z, -y
    np.testing.assert_allclose(g, [gx, 0, 0, 0, gx * 0.25, -gx * 0.25], rtol=1e-14, atol=1e-14 * abs(gx))
    # the gradient is the derivative of the score (away from the snap of small angles and from the float pose matrix:
    # translations that are exact floats)
    h = 2.0 ** -12
    s = NR.shape("slab")
    mdl = NR.model(s.tgt, s.res)
    src = s.src[:300]
    g0 = NR.score_gradient(src, np.zeros(6), mdl, s.res)[1]
    for k in range(3):
        d = np.zeros(6)
        d[k] = h
        fd = (NR.score_gradient(src, d, mdl, s.res)[0] - NR.score_gradient(src, -d, mdl, s.res)[0]) / (2 * h)
        assert abs(fd - g0[k]) <= 2e-3 * np.abs(g0[:3]).max(), (k, fd, g0[k])
