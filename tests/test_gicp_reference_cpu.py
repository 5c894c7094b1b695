"""The checker of the GICP stress tests, checked: tests/gicp_reference.py's numpy statement of the pairs, the Mahalanobis
matrices and both objectives against the C oracle (oracle/gicp.c) on every stress case and state -- two independent
statements (a brute force against a kd-tree; an adjugate in long double against Eigen's cofactor order in double; per-pair
long double sums against double-double ones and, for the statistics objective, against the 74 sums; rotation derivatives
from elementary rotations against PCL's table) --, the reference held to what can be known without either (an inverse
times its argument, a cloud against itself, its own finite differences), and the cases held to what they claim.

What the oracle's distance from the reference turned out to be (printed with -s, recorded in gicp_reference.py as
REF_VS_ORACLE_*): a few units in the last place of f and of the largest gradient entry on EVERY case and state, both
objectives -- also after the rotation step of 1e-4 rad, 55 km from the origin as next to it.  (A comparison that forms
T(x) by rounding the double matrix of x to float, instead of from float sines and cosines by float products as
applyState does, is 1e-8 off there: that is one ulp of the matrix's entries, not the expansion.)"""
import numpy as np
import pytest

import gicp_reference as GR
import knn_reference as KR

LD = np.longdouble
_cov = {}


def _setup(oracle, name):
    """the oracle's covariances (zero rows at non-finite points), the reference's pairs and Mahalanobis matrices: once"""
    if name not in _cov:
        c = GR.case(name)
        src, tgt = c.finite()
        fs, ft = np.isfinite(c.src).all(1), np.isfinite(c.tgt).all(1)
        C1, C2 = np.zeros((len(c.src), 3, 3)), np.zeros((len(c.tgt), 3, 3))
        C1[fs], C2[ft] = oracle.gicp_covariances(src), oracle.gicp_covariances(tgt)
        idx, _ = c.pairs()
        si = np.nonzero(idx >= 0)[0].astype(np.int32)
        _cov[name] = (C1, C2, si, idx[si], GR.mahal_of_pairs(C1, C2, idx, c.T0f))
    return _cov[name]


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    print("\nworst distance of the oracle from the numpy reference, relative to |f| / to the largest gradient entry:")
    for key in sorted(w):
        print("    %-10s %-13s f %.3g (%s)   g %.3g (%s)" % (key + w[key]["f"] + w[key]["g"]))


# --------------------------------------------------------------------------------------------------- the pairs
@pytest.mark.parametrize("name", GR.NAMES)
def test_pairs_equal_the_oracles_kdtree_and_gate(oracle, name):
    c = GR.case(name)
    src, tgt = c.finite()
    fs, ft = np.nonzero(np.isfinite(c.src).all(1))[0], np.nonzero(np.isfinite(c.tgt).all(1))[0]
    oi, od = oracle.KdTree(tgt).nn(oracle.transform_cloud_f(src, c.T0f))
    keep = od.astype(np.float64) < c.max_corr * c.max_corr
    want = np.full(len(c.src), -1, np.int32)
    want[fs] = np.where(keep, ft[oi], -1)
    idx, d2 = c.pairs()
    assert np.array_equal(idx, want)
    assert np.array_equal(d2[fs][keep], od[keep]) and not d2[idx < 0].any()


def test_equal_distances_go_to_the_lowest_index():
    tgt = np.float32([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 0.5]])
    src = np.float32([[0, 0, 0], [0, 0.9, 0], [0, np.inf, 0], [9, 9, 9]])
    idx, d2 = GR.pairs(src, tgt, np.eye(4), 1.0)
    assert idx.tolist() == [5, 1, -1, -1]  # 0.25 < 1; rows 1 and 3 tie; not a query; nothing within 1
    idx, d2 = GR.pairs(src, tgt[:5], np.eye(4), 1.0)
    assert idx.tolist() == [-1, 1, -1, -1]  # four candidates at d2 = 1 exactly: the gate is strict
    idx, d2 = GR.pairs(src, tgt[:5], np.eye(4), 1.0000001)
    assert idx.tolist() == [0, 1, -1, -1] and d2[0] == 1.0


# ------------------------------------------------------------------------------------ the reference on its own
def test_mahalanobis_times_its_argument_is_the_identity(oracle):
    worst = 0.0
    for name in ("scene", "point", "dups", "line", "exact_plane", "utm"):
        c = GR.case(name)
        C1, C2, si, ti, _ = _setup(oracle, name)
        R = c.T0f[:3, :3].astype(np.float64)
        M = GR.mahalanobis(C1[si], C2[ti], R)
        S = C2[ti].astype(LD) + np.einsum("ab,nbc,dc->nad", R.astype(LD), C1[si].astype(LD), R.astype(LD))
        worst = max(worst, float(np.abs(np.einsum("nab,nbc->nac", M, S) - np.eye(3)).max()),
                    float(np.abs(np.einsum("nab,nbc->nac", S, M) - np.eye(3)).max()))
    print("mahalanobis: |M S - I| worst %.3g" % worst)
    assert worst <= 1e-13


def test_a_cloud_against_itself_at_the_identity(oracle):
    for name in ("scene", "dups", "utm", "holes"):
        cloud = KR.shapes()[name]
        idx, d2 = GR.pairs(cloud, cloud, np.eye(4), GR.MAX_CORR)
        fin = np.isfinite(cloud).all(1)
        assert (idx >= 0).sum() == fin.sum() and not d2.any()
        if name != "dups":  # (a triple's lowest index)
            assert np.array_equal(idx[fin], np.nonzero(fin)[0])
        C = np.zeros((len(cloud), 3, 3))
        C[fin] = oracle.gicp_covariances(cloud[fin])
        M = GR.mahal_of_pairs(C, C, idx, np.eye(4))
        si = np.nonzero(idx >= 0)[0]
        for f, g in (GR.fdf_pcl(cloud, cloud, si, idx[si], M, np.zeros(6)),
                     GR.fdf_statistics(cloud, cloud, si, idx[si], M, np.eye(4), np.zeros(6))):
            assert f == 0.0 and not g.any()


@pytest.mark.parametrize("name", ["scene", "half", "clumps_outliers", "utm", "three_pairs", "n65"])
def test_statistics_gradient_is_the_derivative_of_its_own_f(oracle, name):
    """central differences in long double of the smooth form (the exact matrix of x in place of PCL's float one), at the
    rotated state; each block of the gradient relative to ITS largest entry (utm's angles weigh 1e5 times its metres)"""
    c = GR.case(name)
    _, _, si, ti, M = _setup(oracle, name)
    x = c.states[2]

    def f_ld(y):  # f itself in long double: fdf_statistics rounds its results to double
        r0 = (GR.transform_f(c.T0f, c.src[si]) - c.tgt[ti]).astype(LD)
        W = np.c_[GR.rotation(y)[0], np.asarray(y[:3]).astype(LD)]
        D = W - c.T0f[:3].astype(LD)
        p = c.src[si].astype(LD)
        r = r0 + p @ D[:, :3].T + D[:, 3]
        Ms = (M[si].astype(LD) + M[si].transpose(0, 2, 1).astype(LD)) / 2
        return np.einsum("na,nab,nb->n", r, Ms, r).sum() / len(si)

    f, g = GR.fdf_statistics(c.src, c.tgt, si, ti, M, c.T0f, x, float_matrix=False)
    assert abs(f - float(f_ld(x.astype(LD)))) <= 1e-15 * abs(f)
    fd = np.zeros(6)
    for k in range(6):
        h = np.zeros(6, LD)
        h[k] = LD(2.0) ** -20
        fd[k] = float((f_ld(x.astype(LD) + h) - f_ld(x.astype(LD) - h)) / (2 * h[k]))
    for block in (slice(0, 3), slice(3, 6)):
        scale = np.abs(g[block]).max()
        assert np.abs(fd[block] - g[block]).max() <= 1e-9 * scale, (name, fd, g)
    # and with PCL's float matrix the same gradient formula, at the matrix that x rounds to: close to the smooth one's
    _, gf = GR.fdf_statistics(c.src, c.tgt, si, ti, M, c.T0f, x)
    for block in (slice(0, 3), slice(3, 6)):
        assert np.abs(gf[block] - g[block]).max() <= 1e-3 * np.abs(g[block]).max()


@pytest.mark.parametrize("name", [n for n in GR.NAMES if n != "no_pair"])
def test_pcl_gradient_is_the_statistics_gradient_at_the_pairing_pose(oracle, name):
    """PCL's function is not smooth (the float transform of every point) -- but at the pairing pose T(x0) = T0 the two
    objectives are the same residuals: the same f, and the same gradient up to M's asymmetry (the rounding of an
    inverse)"""
    c = GR.case(name)
    _, _, si, ti, M = _setup(oracle, name)
    assert np.array_equal(GR.matrix_f(c.states[0]), c.T0f)
    fp, gp = GR.fdf_pcl(c.src, c.tgt, si, ti, M, c.states[0])
    fs, gs = GR.fdf_statistics(c.src, c.tgt, si, ti, M, c.T0f, c.states[0])
    assert fp > 0 and abs(fp - fs) <= 1e-14 * fp
    assert np.abs(gp - gs).max() <= 1e-12 * np.abs(gs).max()


# ------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", [n for n in GR.NAMES if n != "no_pair"])
def test_oracle_objectives_sit_within_twice_the_recorded_distance(oracle, worst, name):
    c = GR.case(name)
    _, _, si, ti, M = _setup(oracle, name)
    failures = []
    for k, x in enumerate(c.states):
        of, og = oracle.gicp_fdf(c.src, c.tgt, si, ti, M, np.eye(4), x)
        rf, rg = GR.fdf_pcl(c.src, c.tgt, si, ti, M, x)
        qf, qg, Q = oracle.gicp_fdf_statistics(c.src, c.tgt, si, ti, M, np.eye(4), c.T0f, x)
        sf, sg = GR.fdf_statistics(c.src, c.tgt, si, ti, M, c.T0f, x)
        assert Q[73] == len(si) and rf > 0 and sf > 0
        for obj, (a, ga), (b, gb) in (("pcl_sums", (of, og), (rf, rg)), ("statistics", (qf, qg), (sf, sg))):
            e_f, e_g = abs(a - b) / abs(b), float(np.abs(ga - gb).max() / np.abs(gb).max())
            group = GR.group_of(c, k) if obj == "statistics" else GR.group_of(c, 0)
            w = worst.setdefault((obj, group), {"f": (0.0, ""), "g": (0.0, "")})
            if e_f >= w["f"][0]:
                w["f"] = (e_f, name)
            if e_g >= w["g"][0]:
                w["g"] = (e_g, name)
            b_f, b_g = GR.ref_vs_oracle(obj, c, k)
            print("%s state %d %s: f %.17g  oracle off by %.2e (f) %.2e (g)" % (name, k, obj, b, e_f, e_g))
            if not (e_f <= 2 * b_f and e_g <= 2 * b_g):
                failures.append((name, k, obj, e_f, e_g))
    assert not failures, failures


@pytest.mark.parametrize("name", [n for n in GR.NAMES if n != "no_pair"])
def test_oracle_gives_the_same_bits_in_any_pair_order(oracle, name):
    """what every bit-for-bit contract of the device paths rests on: the double-double sums round to the same double
    however the pairs are dealt out -- on every stress case, 20 random orders, every state"""
    c = GR.case(name)
    _, _, si, ti, M = _setup(oracle, name)
    for x in c.states:
        f0, g0 = oracle.gicp_fdf(c.src, c.tgt, si, ti, M, np.eye(4), x)
        q0, h0, Q0 = oracle.gicp_fdf_statistics(c.src, c.tgt, si, ti, M, np.eye(4), c.T0f, x)
        for seed in range(20):
            pm = np.random.default_rng(seed).permutation(len(si))
            f1, g1 = oracle.gicp_fdf(c.src, c.tgt, si[pm], ti[pm], M, np.eye(4), x)
            q1, h1, Q1 = oracle.gicp_fdf_statistics(c.src, c.tgt, si[pm], ti[pm], M, np.eye(4), c.T0f, x)
            assert f1 == f0 and np.array_equal(g1, g0), (name, seed)
            assert q1 == q0 and np.array_equal(h1, h0) and np.array_equal(Q1, Q0), (name, seed)


@pytest.mark.parametrize("name", GR.NAMES)
def test_oracle_registration_starts_from_the_references_pairs(oracle, name):
    """the gate and the tie rule inside wmo_gicp_align: one forced iteration reports the pairs of the first search, under
    the identity -- where `half_start` has one point exactly on the gate"""
    c = GR.case(name)
    src, tgt = c.finite()
    max_corr = c.max_corr
    idx, d2 = GR.pairs(src, tgt, np.eye(4), max_corr)
    if name == "half_start":
        _, far = GR.pairs(src, tgt, np.eye(4), 1e3)
        assert (far.astype(np.float64) == max_corr * max_corr).sum() == 1 and 0.4 <= (idx < 0).mean() <= 0.6
    got = oracle.gicp_align(src, tgt, max_corr=max_corr, force_iterations=1)
    assert got["n_corr"] == (idx >= 0).sum(), (name, got["n_corr"], (idx >= 0).sum())
    assert got["converged"] == (got["n_corr"] >= 4) and got["iterations"] == int(got["converged"])


# -------------------------------------------------------------------------------------------------- the cases
def test_cases_hold_what_they_name():
    C = GR.cases()
    counts = {name: int((c.pairs()[0] >= 0).sum()) for name, c in C.items()}
    for name in KR.NAMES:  # every finite source point finds its own image (or a nearer point) within 5 m -- utm* too
        assert counts[name] == np.isfinite(C[name].src).all(1).sum(), name
        assert np.array_equal(C[name].src, KR.shapes()[name], equal_nan=True)
    for name in ("utm", "utm_plane"):  # ... under the motion's own state: its angles about the ORIGIN leave no pair at all
        c = C[name]
        about_origin = GR.matrix_f(np.r_[GR.PAIR_X[:3], c.x0[3:]])
        assert np.abs(c.x0[:3]).max() > 50.0 and np.abs(c.x0[3:]).min() > 5e-4
        assert (GR.pairs(c.src, c.tgt, about_origin, c.max_corr)[0] >= 0).sum() == 0
    assert (counts["no_pair"], counts["one_pair"], counts["three_pairs"], counts["four_pairs"]) == (0, 1, 3, 4)
    # half: 40 to 60 % unmatched, interleaved by index, and one point exactly ON the gate (not a pair)
    h = C["half"]
    idx, _ = h.pairs()
    un = idx < 0
    assert 0.4 <= un.mean() <= 0.6
    assert (un[1:] != un[:-1]).sum() > len(un) // 4 and un[:64].any() and not un[:64].all()
    _, d2 = GR.pairs(h.src, h.tgt, h.T0f, 1e3)
    on = d2.astype(np.float64) == h.max_corr * h.max_corr
    assert on.sum() == 1 and un[on].all()
    # holes_both: non-finite rows on both sides, two rows bad on both, bad rows at either end
    b = C["holes_both"]
    bs, bt = ~np.isfinite(b.src).all(1), ~np.isfinite(b.tgt).all(1)
    assert bs.sum() == 4 and bt.sum() == 4 and (bs & bt).sum() == 2 and bs[0] and bs[-1] and bt[-1]
    assert np.isnan(b.tgt).any() and np.isposinf(b.tgt).any() and np.isneginf(b.tgt).any()
    assert counts["holes_both"] == 2996 and (b.pairs()[0][bs] == -1).all() and not np.isin(b.pairs()[0], np.nonzero(bt)[0]).any()
    for n in GR.SIZES:
        c = C["n%d" % n]
        assert len(c.src) == n == counts["n%d" % n] and len(c.tgt) == 3000
    # lattice: the motion leaves no exact tie, dups and point: every match is one of equal candidates
    for name in ("dups", "point"):
        c = C[name]
        idx, _ = c.pairs()
        first = np.array([np.nonzero((c.tgt == c.tgt[j]).all(1))[0][0] for j in idx[:200]])
        assert np.array_equal(idx[:200], first) and (np.unique(c.tgt, axis=0).shape[0] < len(c.tgt))
    assert max(len(c.src) for c in C.values()) <= 3375 and max(len(c.tgt) for c in C.values()) <= 3375
