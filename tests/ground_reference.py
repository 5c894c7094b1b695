"""An independent float64 restatement of libwave's Gaussian-process ground filter,
wave::GroundSegmentation<PointT>::applyFilter (wave_matching/include/wave/matching/impl/
ground_segmentation.hpp:358-381), written from the reference's text with numpy.  It shares no code
with the HIP kernels (libwave_amd/csrc/wm_ground.hip): the GP solves here are LU solves of the whole
matrix (np.linalg.solve), where the device extends a Cholesky factor row by row.

What the reference does, line by line (impl = impl/ground_segmentation.hpp):

Binning, per point in input order (impl :36-84).
  * in range iff sqrt(px*px + py*py + pz*pz) < rmax: the products and sums in float, the unqualified
    sqrt read as the C library's double sqrt, compared with the double rmax (:48).  NaN / inf points
    fail the test and get no label.
  * sector = (unsigned)(wrapTo360(atan2(py, px) * (180 / M_PI)) / (360.0 / num_bins_a)), all in double,
    the constant 180 / M_PI formed first (:39, :49-55); wrapTo360 is wave_utils/src/math.cpp:80-87
    (x > 0: fmod(x, 360), else fmod(x + 360, 360)).
  * linear bin = (unsigned)(xy / (rmax / num_bins_l)) with xy = std::sqrt(px*px + py*py) in float (:40,
    :58-61).
  * the cell's prototype is its lowest-z point: a strict `<` over ascending index, so a tie keeps the first
    index (:71-72); the signal point is (range = xy of the prototype, height = its z) (:76-80).
Signal cells (:117-135): only cells that hold MORE than 5 points (:123).
Seeds (:138-186).
  * the sector's signal points are sorted by height (:138);
  * walked in order, a point is a seed iff range < max_seed_range and |height| < max_seed_height (:159-160);
    the walk stops after min(size, num_seed_points) seeds (:143-146, :175);
  * the loop takes one eligible seed BEFORE it checks the count (:153-179): num_seed_points = 0 takes the
    lowest signal point if it is eligible, nothing otherwise; a negative num_seed_points becomes a huge
    size_t, so every eligible point is a seed;
  * fewer than 2 seeds (:182-186): the seed cells are still labelled (against their own heights), every
    other cell of the sector is left unlabelled (sufficient_model = false, :328).
INSAC passes (:202-286).
  * f_s = C_XsX (C_XX + p_sn I)^-1 z, Vf_s = C_XsXs - C_XsX (C_XX + p_sn I)^-1 C_XXs; the kernel is
    p_sf * exp(coeff * d^2) with float coeff = -1 / (2 p_l^2) (:87-105, :205-226).  Double arithmetic;
    each float parameter enters as its float value.
  * every remaining point is tested against the pass-start model: an inlier iff vf < p_tmodel and
    |h - f| / sqrt(p_sn + vf * vf) < p_tdata (:240-246; vf squared, as written);
  * inliers move to the end of the model in their current order (:247-249);
  * passes repeat until a pass adds nothing or no point remains (:281-285).  Only diag(Vf_s) is read.
Labels (:288-354).
  * model cells: float h = |model_height - z|; h < p_tg ground, else h > robot_height overhanging, else
    obstacle (:302-319);
  * the remaining signal cells, only when the model is sufficient: float h = |z - f_s(i)| with the last
    pass's prediction; h > robot_height overhanging, else obstacle -- never ground (:328-353).
Output order (:290-381): each list is ordered by sector; within a sector model cells first (model order:
seeds, then each pass's inliers), then the remaining cells in ascending height; within a cell, input index
order.  The output is ground, obstacle, overhanging -- each list only if kept (:366-380).
`max_bin_points` is parsed but never used.

Defined here where the reference is undefined:
  (a) height ties: std::sort is not stable -- ties are broken by ascending linear-bin index;
  (b) a bin index that rounds up to num_bins_a / num_bins_l is clamped to the last bin;
  (c) every call classifies its input afresh (the reference never clears its index vectors);
  (d) atan2 / sqrt are the C library's double functions; -0.0 ties with +0.0 in the prototype search.

segment() also returns the MINIMUM DECISION MARGIN: the smallest relative distance of any vf / p_tmodel,
|met| / p_tdata or prediction-based h / robot_height comparison from its threshold -- the only comparisons
where a Cholesky solve and an LU solve can disagree (the float rounding of h is taken into account: the
threshold is the double value at which float(h) crosses robot_height).  And the BINNING MARGIN: the
smallest distance of an in-range point's ph / bsize_rad from an integer -- the one place where the device's
atan2 and numpy's can disagree in the last bit (a point on an axis, x == 0 or y == 0, is left out: atan2 is
exact there in both libraries).  EXACT_MARGIN, the smallest distance of an in-range xy / bsize_lin from an
integer (xy != 0) and of any finite point's radius from rmax (relative), is reported for information only:
xy and the radius are correctly rounded square roots and the divisions IEEE ones on both sides, so they cannot
differ (the fixture holds points with xy exactly 5.0 m, ratio 10, and one at radius exactly 5.0 m).
"""
import math

import numpy as np

NONE, GROUND, OBSTACLE, OVERHANGING = 0, 1, 2, 3
KEEP_GROUND, KEEP_OBSTACLE, KEEP_OVERHANGING = 1, 2, 4
KEEP_DEFAULT = KEEP_OBSTACLE | KEEP_OVERHANGING  # keep_ground = false, keep_obs = keep_drv = true

_FLOAT = ("p_l", "p_sf", "p_sn", "p_tmodel", "p_tdata", "p_tg")
_INT = ("max_bin_points", "num_seed_points", "num_bins_a", "num_bins_l")
_DOUBLE = ("rmax", "robot_height", "max_seed_range", "max_seed_height")

# YAML key -> field (ground_segmentation_params.hpp:44-57)
YAML_KEYS = {"rmax": "rmax", "num_maxbinpoints": "max_bin_points", "num_seedpoints": "num_seed_points",
             "num_ang_bins": "num_bins_a", "num_lin_bins": "num_bins_l", "gp_lengthparameter": "p_l",
             "gp_covariancescale": "p_sf", "gp_modelnoise": "p_sn", "gp_groundmodelconfidence": "p_tmodel",
             "gp_grounddataconfidence": "p_tdata", "gp_groundthreshold": "p_tg", "robotheight": "robot_height",
             "seeding_maxrange": "max_seed_range", "seeding_maxheight": "max_seed_height"}


def default_params():
    """GroundSegmentationParams' defaults (ground_segmentation_params.hpp:10-36)."""
    return dict(rmax=100.0, max_bin_points=200, num_seed_points=10, p_l=4.0, p_sf=1.0, p_sn=0.3, p_tmodel=5.0,
                p_tdata=5.0, p_tg=0.3, robot_height=1.2, max_seed_range=50.0, max_seed_height=15.0,
                num_bins_a=72, num_bins_l=200)


def load_yaml(path):
    """The 14 keys of the reference's YAML constructor (flat `key: value  # comment` file)."""
    p = default_params()
    for line in open(path):
        line = line.split("#", 1)[0].strip()
        if ":" not in line:
            continue
        k, v = (s.strip() for s in line.split(":", 1))
        if k in YAML_KEYS:
            f = YAML_KEYS[k]
            p[f] = int(v) if f in _INT else float(v)
    return p


def params_valid(p):
    """What the C ABI rejects with WM_ERR_ARG: parameters that would make the reference index out of bounds or
    divide into NaN."""
    for k in _FLOAT:
        if not math.isfinite(float(np.float32(p[k]))):
            return False
    for k in _DOUBLE:
        if not math.isfinite(float(p[k])):
            return False
    return (p["num_bins_a"] > 0 and p["num_bins_l"] > 0 and np.float32(p["p_l"]) > 0
            and np.float32(p["p_sf"]) > 0 and np.float32(p["p_sn"]) > 0)


def _threshold_after_float_rounding(t):
    """The double value at which float(h) > t (t a double) flips: h >= it  <=>  float(h) > t (up to the tie)."""
    f = np.float32(t)
    hi = f if float(f) > t else np.nextafter(f, np.float32(np.inf))
    lo = np.nextafter(hi, np.float32(-np.inf))
    return (float(lo) + float(hi)) / 2.0


def segment(pts, params=None, keep=KEEP_DEFAULT):
    """-> dict(labels (n,) uint8, ground / obstacle / overhanging (int32, ordered), indices (the kept lists
    concatenated), stats, margin (decisions), bin_margin, exact_margin, factor_rows / extended_from (the largest model a pass
    solved with / the largest factor a later pass extended), cell (per point, -1: out of range),
    prototype (per cell, -1: empty))."""
    P = default_params() if params is None else dict(params)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    A, L = int(P["num_bins_a"]), int(P["num_bins_l"])
    rmax = float(P["rmax"])
    f32 = {k: np.float32(P[k]) for k in _FLOAT}
    p_sf, p_sn = float(f32["p_sf"]), float(f32["p_sn"])
    p_tmodel, p_tdata, p_tg = float(f32["p_tmodel"]), float(f32["p_tdata"]), f32["p_tg"]
    rh = float(P["robot_height"])
    coeff = float(np.float32(-1.0) / (np.float32(2.0) * f32["p_l"] * f32["p_l"]))
    nsp = int(P["num_seed_points"])

    # ---- binning (impl :36-84)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = (x * x + y * y) + z * z                      # float
        rad = np.sqrt(r2.astype(np.float64))               # C's double sqrt
        inr = rad < rmax
        xy = np.sqrt(x * x + y * y)                        # float std::sqrt
    idx = np.nonzero(inr)[0]
    bsize_rad = 360.0 / A
    bsize_lin = rmax / L
    margin_bin = margin_exact = math.inf
    sector = np.zeros(0, np.int64)
    lin = np.zeros(0, np.int64)
    if len(idx):
        xi, yi = x[idx].astype(np.float64), y[idx].astype(np.float64)
        ph = np.arctan2(yi, xi) * (180.0 / math.pi)
        ph = np.where(ph > 0, np.fmod(ph, 360.0), np.fmod(ph + 360.0, 360.0))   # wrapTo360
        q_rad = ph / bsize_rad
        q_lin = xy[idx].astype(np.float64) / bsize_lin
        sector = np.minimum(q_rad.astype(np.int64), A - 1)   # (b) clamp
        lin = np.minimum(q_lin.astype(np.int64), L - 1)
        inexact = (xi != 0) & (yi != 0)
        if inexact.any():
            d = np.abs(q_rad[inexact] - np.rint(q_rad[inexact]))
            margin_bin = min(margin_bin, float(d.min()))
        nz = xy[idx] != 0
        if nz.any():
            d = np.abs(q_lin[nz] - np.rint(q_lin[nz]))
            margin_exact = float(d.min())
    fin = np.isfinite(rad)
    if fin.any() and rmax > 0:
        margin_exact = min(margin_exact, float(np.min(np.abs(rad[fin] - rmax))) / rmax)

    C = A * L
    cell = sector * L + lin                                  # per in-range point (input order)
    counts = np.bincount(cell, minlength=C) if len(idx) else np.zeros(C, np.int64)
    # points of every cell in ascending input index
    order = np.argsort(cell, kind="stable")
    cell_sorted = cell[order]
    pts_sorted = idx[order]
    starts = np.searchsorted(cell_sorted, np.arange(C + 1))
    # prototype: lowest z, first index on a tie; -0.0 == +0.0 ((d): z + 0.0 turns -0.0 into +0.0)
    proto = np.full(C, -1, np.int64)
    if len(idx):
        zc = z[idx].astype(np.float64) + 0.0
        o = np.lexsort((idx, zc, cell))
        first = np.ones(len(o), bool)
        first[1:] = cell[o][1:] != cell[o][:-1]
        proto[cell[o][first]] = idx[o][first]

    labels = np.zeros(n, np.uint8)
    lists = {GROUND: [], OBSTACLE: [], OVERHANGING: []}
    st = dict(n_in_range=int(len(idx)), n_signal_cells=0, n_model_cells=0, n_sufficient_sectors=0,
              passes_total=0, passes_max=0)
    factor_rows = 0     # the largest model a pass started from (the rows of the factor it solved with)
    extended_from = 0   # the largest model a pass extended (model size at the start of a pass after the first)
    margin = math.inf
    rh_eff = _threshold_after_float_rounding(rh)

    def rel(a, t):
        return abs(a - t) / abs(t) if t != 0 else abs(a - t)

    for s in range(A):
        bins = np.nonzero(counts[s * L:(s + 1) * L] > 5)[0]
        if len(bins) == 0:
            continue
        st["n_signal_cells"] += len(bins)
        pr = proto[s * L + bins]
        rng_ = xy[pr].astype(np.float64)
        hgt = z[pr].astype(np.float64)
        o = np.lexsort((bins, hgt))                     # (a) height, then bin
        sig = [(float(rng_[k]), float(hgt[k]), int(bins[k])) for k in o]
        # seeds (:143-179)
        num_points = len(sig) if nsp < 0 else min(len(sig), nsp)
        model, cur, count = [], 0, 0
        while True:
            if cur >= len(sig):
                break
            if sig[cur][0] < P["max_seed_range"] and abs(sig[cur][1]) < P["max_seed_height"]:
                model.append(sig.pop(cur))
                count += 1
            else:
                cur += 1
            if count >= num_points:
                break
        sufficient = len(model) >= 2
        keep_going = sufficient and len(sig) > 0
        f_last = None
        passes = 0
        while keep_going:
            passes += 1
            factor_rows = max(factor_rows, len(model))
            if passes > 1:
                extended_from = max(extended_from, prev_start)
            prev_start = len(model)
            mr = np.array([m[0] for m in model])
            mz = np.array([m[1] for m in model])
            rr = np.array([q[0] for q in sig])
            rz = np.array([q[1] for q in sig])
            d = mr[:, None] - mr[None, :]
            K = p_sf * np.exp(coeff * (d * d)) + p_sn * np.eye(len(mr))
            d = rr[:, None] - mr[None, :]
            Cx = p_sf * np.exp(coeff * (d * d))
            sol = np.linalg.solve(K, np.concatenate([Cx.T, mz[:, None]], axis=1))
            f = Cx @ sol[:, -1]
            vf = p_sf - np.sum(Cx * sol[:, :-1].T, axis=1)
            met = (rz - f) / np.sqrt(p_sn + vf * vf)
            ok_v = vf < p_tmodel
            inl = ok_v & (np.abs(met) < p_tdata)
            for k in range(len(sig)):
                margin = min(margin, rel(vf[k], p_tmodel))
                if ok_v[k]:
                    margin = min(margin, rel(abs(met[k]), p_tdata))
            added = [sig[k] for k in range(len(sig)) if inl[k]]
            sig = [sig[k] for k in range(len(sig)) if not inl[k]]
            f_last = f[~inl]
            model += added
            if not added or not sig:
                keep_going = False
        st["passes_total"] += passes
        st["passes_max"] = max(st["passes_max"], passes)
        st["n_model_cells"] += len(model)
        st["n_sufficient_sectors"] += int(sufficient)
        sec = {GROUND: [], OBSTACLE: [], OVERHANGING: []}
        for (_, mh, b) in model:
            c = s * L + b
            js = pts_sorted[starts[c]:starts[c + 1]]
            h = np.abs(mh - z[js].astype(np.float64)).astype(np.float32)
            lab = np.where(h < p_tg, GROUND, np.where(h.astype(np.float64) > rh, OVERHANGING, OBSTACLE))
            labels[js] = lab
            for l_ in (GROUND, OBSTACLE, OVERHANGING):
                sec[l_].append(js[lab == l_])
        if sufficient and sig:
            for k, (_, _, b) in enumerate(sig):
                c = s * L + b
                js = pts_sorted[starts[c]:starts[c + 1]]
                hd = np.abs(z[js].astype(np.float64) - f_last[k])
                margin = min(margin, float(np.min(np.abs(hd - rh_eff))) / abs(rh) if rh != 0 else math.inf)
                h = hd.astype(np.float32)
                lab = np.where(h.astype(np.float64) > rh, OVERHANGING, OBSTACLE)
                labels[js] = lab
                for l_ in (OBSTACLE, OVERHANGING):
                    sec[l_].append(js[lab == l_])
        for l_ in sec:
            lists[l_] += sec[l_]
    out = {}
    for l_, name in ((GROUND, "ground"), (OBSTACLE, "obstacle"), (OVERHANGING, "overhanging")):
        out[name] = (np.concatenate(lists[l_]) if lists[l_] else np.zeros(0, np.int64)).astype(np.int32)
    kept = []
    if keep & KEEP_GROUND:
        kept.append(out["ground"])
    if keep & KEEP_OBSTACLE:
        kept.append(out["obstacle"])
    if keep & KEEP_OVERHANGING:
        kept.append(out["overhanging"])
    out["indices"] = np.concatenate(kept).astype(np.int32) if kept else np.zeros(0, np.int32)
    st["n_ground"], st["n_obstacle"], st["n_overhanging"] = (len(out["ground"]), len(out["obstacle"]),
                                                            len(out["overhanging"]))
    out["labels"] = labels
    out["cell"] = np.full(n, -1, np.int64)
    out["cell"][idx] = cell
    out["prototype"] = proto
    out["stats"] = st
    out["margin"] = margin
    out["bin_margin"] = margin_bin
    out["exact_margin"] = margin_exact
    out["factor_rows"] = factor_rows
    out["extended_from"] = extended_from
    return out


def car_box_removal(pts):
    """The reference test's pcl::ConditionalRemoval (tests/ground_segmentation_test.cpp:26-52): keep a point iff
    (x < -3 or x > 3) or (y < -1.1 or y > 1.1); NaN coordinates fail every comparison."""
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore"):
        m = (x < -3) | (x > 3) | (y < np.float32(-1.1)) | (y > np.float32(1.1))
    return np.ascontiguousarray(pts[m])
