"""tests/fpfh_radius_reference.py checked itself, on the CPU (no GPU): the kd-tree variant against the brute-force one;
the rule against a literal float64 restatement of PCL (fpfh_reference's pair features in float64, 1 / d2 weights and
double sums); the arithmetic edges of the rule (x and e, the weight's range, the int64 bounds); the entry points'
argument errors before a device is touched.

Figures of the three clouds (FR.clouds(), 6 000 points) at a feature radius of 6 / 10 median spacings, the normal radius
half of it, measured here with the reference alone:
  feature neighbours (the point included)  median 27 / 17 / 13, maxima 64 / 167 / 136 at 6 x; 73 / 49 / 34 and
                                           138 / 320 / 305 at 10 x
  ambiguous pairs (a bin coordinate within 1e-4 of a decision, or a swap within 1e-4 that changes a bin)
                                           below 5 % on every cloud and radius (printed)
  points with an f1-risky pair             1.00 / 0.25 / 1.53 % at 6 x, 1.43 / 0.27 / 1.72 % at 10 x: RR.RISKY_SHARE holds
                                           the largest per radius, the device test's cap is that plus one percentage
                                           point.  10 x stays below 4 %, so 10 x it is (not 8 x).
  points with a neighbour nearer than r / 256 (left out of the row comparison): 0.00 - 0.13 %."""
import ctypes as C
import os

import numpy as np
import pytest

import fpfh_radius_reference as RR
import fpfh_reference as FR
import iss_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = ["scene", "rings", "scan"]
MAX_LEFT_OUT = 0.05  # the k form's CPU bound
ROW_REL = 2e-6


def _small_cases():
    out = {}
    for name in CLOUDS:
        c = FR.clouds()[name][:700]
        s = IR.median_spacing(c)
        out[name] = (c, 3.0 * s, 6.0 * s)
    d = IR.dense_cloud(193)
    for n in (1, 2, 3, 65, 193):
        out["dense-%d" % n] = (d[:n], 0.6, 1.0)
    sub = FR.clouds()["scan"][:400]
    s = IR.median_spacing(sub)
    bad = sub.copy()
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    out["nan-inf"] = (bad, 3.0 * s, 6.0 * s)
    out["duplicates"] = (np.r_[sub[:200], sub[:200]], 3.0 * s, 6.0 * s)
    out["all-nan"] = (np.full((9, 3), np.nan, np.float32), 0.5, 1.0)
    return out


@pytest.mark.parametrize("case", sorted(_small_cases()))
def test_the_kdtree_variant_equals_the_brute_one(case):
    cloud, rn, rf = _small_cases()[case]
    a, b = RR.normal_sums(cloud, rn), RR.normal_sums(cloud, rn, brute=True)
    assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["counts"], b["counts"]) and a["x"] == b["x"]
    nrm = RR.normals(cloud, rn)[0]
    ca, oa, na, ra = RR.fpfh(cloud, nrm, rf)
    cb, ob, nb, rb = RR.fpfh(cloud, nrm, rf, brute=True)
    assert np.array_equal(ca, cb) and np.array_equal(na, nb) and np.array_equal(ra, rb)
    assert np.array_equal(oa.view(np.uint32), ob.view(np.uint32))
    finite = np.isfinite(cloud).all(1)
    assert np.all(na[~finite] == -1) and np.all(oa[~finite] == 0)
    if finite.sum() > 60:
        assert ca.sum() > 0 and oa.max() > 0


def _setup(name, mult):
    cloud = FR.clouds()[name]
    rn, rf = RR.radii(name, mult)
    nrm = RR.normals(cloud, rn)[0]
    return cloud, nrm, rn, rf


@pytest.mark.parametrize("mult", RR.RADII)
@pytest.mark.parametrize("name", CLOUDS)
def test_rule_gives_pcl_counts_and_rows(name, mult):
    cloud, nrm, rn, rf = _setup(name, mult)
    pairs = RR.feature_pairs(cloud, rf)
    _, _, i, j, d2 = pairs
    n3 = nrm[:, :3]
    rule = FR.pair_features(cloud[i], n3[i], cloud[j], n3[j])
    pcl = FR.pair_features(cloud[i], n3[i], cloud[j], n3[j], dtype=np.float64, pcl=True)
    alt = FR.pair_features(cloud[i], n3[i], cloud[j], n3[j], dtype=np.float64, pcl=True, swap=~pcl["swap"])
    assert np.array_equal(rule["ok"], pcl["ok"])
    use = pcl["ok"]
    close = np.abs(np.abs(pcl["a1"]) - np.abs(pcl["a2"])) < FR.AMBIGUOUS_EPS
    ambiguous = (close & np.any(pcl["bins"] != alt["bins"], axis=-1)) | FR.near_integer(pcl["x1"]) | \
        FR.near_integer(pcl["x2"]) | FR.near_integer(pcl["x3"])
    share = float((ambiguous & use).sum()) / float(use.sum())
    clear = use & ~ambiguous
    assert np.array_equal(rule["bins"][clear], pcl["bins"][clear])
    assert share <= MAX_LEFT_OUT
    # the points the device test may treat as f1-risky
    counts, n_f, risky = RR.spfh(cloud, nrm, rf, pairs_=pairs)
    risky_share = float((risky > 0).mean())
    print("%s %d x: %d pairs, ambiguous %.3f %%; neighbours median %d max %d; f1-risky points %.2f %%" % (
        name, mult, use.sum(), 100 * share, np.median(n_f) + 1, n_f.max() + 1, 100 * risky_share))
    assert risky_share <= RR.RISKY_SHARE[mult] <= 0.04
    # rows: the rule's integer weighting against 1 / d2 in double on the same counts
    out = RR.weight(counts, cloud, nrm, rf, pairs_=pairs)
    lit, near = RR.pcl_weight_literal(counts, cloud, nrm, rf)
    print("%s %d x: points with a neighbour nearer than r / 256: %.2f %%" % (name, mult, 100 * near.mean()))
    assert near.mean() <= MAX_LEFT_OUT
    a, b = out[~near].astype(np.float64), lit[~near]
    assert np.all(np.abs(a - b) <= ROW_REL * b)
    assert (b > 0).sum() > 20 * len(cloud) * 0.5  # (rows with content)
    sums = out.reshape(-1, 3, 11).astype(np.float64).sum(axis=2)
    assert np.all((np.abs(sums - 100) < 1e-3) | (sums == 0))


def test_exponents_for_odd_even_and_negative_x():
    assert [RR.half_exponent(x) for x in (-5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5)] == [-2, -2, -1, -1, 0, 0, 1, 1, 2, 2, 3]
    # radius -> (x, e): r2 = m 2^x with m in [0.5, 1)
    for radius, x, e in ((1.0, 1, 1), (0.5, -1, 0), (0.25, -3, -1), (3.0, 4, 2), (2.0, 3, 2), (0.1, -6, -3), (0.7, -1, 0)):
        r2, gx, ge = RR.exponents(radius)
        assert (gx, ge) == (x, e), radius
        assert 0.5 <= float(r2) * 2.0 ** -gx < 1.0
        # |d| < r < 2^e: a first-moment term stays below 2^36
        assert radius < 2.0 ** ge


def test_weights_and_the_int64_bounds():
    r2 = IR.r2_of(0.7)
    f = np.float32
    d2 = np.array([np.nextafter(r2, f(0)), r2 * f(0.5), r2 * f(2.0 ** -16), r2 * f(2.0 ** -17), f(1e-30)], f)
    W = RR.pair_weights(d2, r2)
    assert W[0] >= 1 << 20 and W[0] <= (1 << 20) + 1  # the weakest weight: ratio just above 1
    assert W[1] == 1 << 21
    assert W[2] == W[3] == W[4] == 1 << 36            # the clamp: nearer than r / 256 weighs as r / 256
    # r / 300 is inside the clamp, r / 200 is not
    assert RR.pair_weights(np.array([f(0.7 / 300) ** 2], f), r2)[0] == 1 << 36
    assert RR.pair_weights(np.array([f(0.7 / 200) ** 2], f), r2)[0] < 1 << 36
    # 8191 neighbours, each with 8191 counts in one bin, each of weight 2^36: one accumulator, and a block's total
    worst = RR.MAX_NEIGHBORS * RR.MAX_NEIGHBORS * (1 << 36)
    assert worst < 1 << 62
    acc = np.zeros(1, np.int64)
    for _ in range(4):
        acc += np.int64(worst // 4)  # (no wrap on the way)
    assert int(acc[0]) == worst // 4 * 4
    # a normal's sums: |d_a d_b| < 1.001 r2 <= 1.001 2^x and |d_c| < 1.001 2^e, so a term is below 1.001 2^36; 2^26 points
    assert int(1.001 * (1 << 36)) * (1 << 26) < 1 << 63


def test_the_option_is_in_the_table():
    src = open(os.path.join(ROOT, "libwave_amd", "csrc", "wm_ctx.hip")).read()
    assert '{"fpfh_cell_div", "WM_TUNE_FPFH_CELL_DIV", nullptr, &wm_ctx::tune_fpfh_cell_div, 0.5, 8, 0}' in src
    assert "`fpfh_cell_div` | `WM_TUNE_FPFH_CELL_DIV` | 2 |" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- the entry points refuse bad arguments before a device is touched (`ctx` is a pointer that must never be followed)

def _call_normals(wm, ctx=C.c_void_p(1), n=10, stride=12, mem=None, out_mem=None, radius=1.0, pts="pts", out="out"):
    a = np.zeros((10, 4), np.float32)
    o = np.full((10, 4), 7.0, np.float32)
    rc = wm.lib().wm_normals_radius(ctx, C.c_void_p(a.ctypes.data) if pts == "pts" else None, n, stride,
                                    wm.WM_MEM_HOST if mem is None else mem, radius, C.c_void_p(o.ctypes.data) if out == "out" else None,
                                    None, None, wm.WM_MEM_HOST if out_mem is None else out_mem, None)
    assert np.all(o == 7.0)  # nothing is written
    return rc


def _call_fpfh(wm, ctx=C.c_void_p(1), n=10, stride=12, mem=None, out_mem=None, params="p", pts="pts", out="out", normals=None,
               normal_radius=0.5, feature_radius=1.0):
    a = np.zeros((10, 4), np.float32)
    o = np.full((10, 33), 7.0, np.float32)
    p = wm.FpfhRadiusParams(normal_radius, feature_radius)
    rc = wm.lib().wm_fpfh_radius(ctx, C.c_void_p(a.ctypes.data) if pts == "pts" else None, n, stride,
                                 wm.WM_MEM_HOST if mem is None else mem, C.byref(p) if params == "p" else None,
                                 C.c_void_p(a.ctypes.data) if normals else None, C.c_void_p(o.ctypes.data) if out == "out" else None,
                                 None, None, wm.WM_MEM_HOST if out_mem is None else out_mem, None)
    assert np.all(o == 7.0)
    return rc


BAD_CLOUD = [dict(ctx=None), dict(pts=None), dict(out=None), dict(stride=8), dict(stride=10), dict(stride=14), dict(mem=5),
             dict(out_mem=7), dict(n=(1 << 26) + 1)]
BAD_RADII = [0.0, -1.0, float("nan"), float("inf"), 1e-20, 1e20]
_ids = lambda b: "-".join("%s=%s" % kv for kv in sorted(b.items()))[:60]  # noqa: E731


@pytest.mark.parametrize("bad", BAD_CLOUD + [dict(radius=r) for r in BAD_RADII], ids=_ids)
def test_normals_radius_argument_errors_without_a_device(wm, bad):
    assert _call_normals(wm, **bad) == wm.WM_ERR_ARG


@pytest.mark.parametrize("bad", BAD_CLOUD + [dict(params=None)] + [dict(feature_radius=r) for r in BAD_RADII] +
                         [dict(normal_radius=r) for r in BAD_RADII] + [dict(feature_radius=r, normals=True) for r in BAD_RADII],
                         ids=_ids)
def test_fpfh_radius_argument_errors_without_a_device(wm, bad):
    assert _call_fpfh(wm, **bad) == wm.WM_ERR_ARG


def test_an_empty_cloud_is_ok_without_a_device(wm):
    assert _call_normals(wm, n=0) == wm.WM_OK
    assert _call_normals(wm, n=0, pts=None) == wm.WM_OK
    assert _call_fpfh(wm, n=0) == wm.WM_OK
    assert _call_fpfh(wm, n=0, pts=None, mem=wm.WM_MEM_DEVICE, out_mem=wm.WM_MEM_DEVICE) == wm.WM_OK
    # a normal radius that is not read may be anything
    assert _call_fpfh(wm, n=0, normals=True, normal_radius=float("nan")) == wm.WM_OK
    assert C.sizeof(wm.FpfhRadiusParams) == 16 and C.sizeof(wm.FpfhRadiusStats) == 40 and wm.WM_FPFH_RADIUS_MAX_NEIGHBORS == 8191
