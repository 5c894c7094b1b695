"""wm_sac_segment_batch (libwave_amd/csrc/wm_sac.hip) on the GPU.  The yardstick is ctx.sac_segment on the same scan
alone, compared BYTE for byte: status, coefficients, indices, labels and every field of the statistics but kernel_ms --
`rounds` included.  tests/test_sac_gpu.py holds the single call to the checker (tests/sac_reference.py); beside it the
batch is compared with the checker directly, without the refit, where the checker has the case."""
import ctypes as C

import numpy as np
import pytest

import sac_reference as SR

pytestmark = pytest.mark.gpu

STATS = ("n_finite", "n_inliers_model", "n_inliers", "iterations", "skipped", "rounds", "refined", "hypotheses",
         "best_hypothesis")
LOOP = ("iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model")
GROUP_A = ("exact_plane", "line", "point", "scene", "holes", "clumps_outliers", "noisy_plane", "utm_plane")
GROUP_B = ("line", "point", "lattice", "dups", "shell")
A = dict(distance_threshold=0.05, max_iterations=50)
B = dict(distance_threshold=0.5, max_iterations=1000)
PERP = dict(model=SR.PERPENDICULAR, axis=(0, 0, 1), eps_angle=0.1)
PAR = dict(model=SR.PARALLEL, axis=(0, 0, 1), eps_angle=0.1)

_SINGLE = {}


def _np(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def _kwkey(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))


def _single(ctx, key, P, **kw):
    """ctx.sac_segment(P, **kw), computed once per (key, kw) and left unchanged"""
    k = (key, _kwkey(kw))
    if k not in _SINGLE:
        got = ctx.sac_segment(P, **kw)
        for f in ("indices", "labels"):
            got[f] = _np(got[f])
        _SINGLE[k] = got
    return _SINGLE[k]


def _same(wm, got, one, what, negative=False):
    assert got["rc"] == one["rc"] and got["rc"] in (wm.WM_OK, wm.WM_NOT_CONVERGED), (what, got["rc"], one["rc"])
    for f in STATS:
        assert got[f] == one[f], (what, f, got[f], one[f])
    assert got["model_coefficients"].tobytes() == one["model_coefficients"].tobytes(), what
    if one["rc"] != wm.WM_OK:
        assert got["coefficients"] is None and got["labels"] is None and len(got["indices"]) == 0 and got["n_out"] == 0, what
        return
    assert got["coefficients"].tobytes() == one["coefficients"].tobytes(), (what, got["coefficients"], one["coefficients"])
    if got["labels"] is not None:
        assert _np(got["labels"]).dtype == np.uint8 and np.array_equal(_np(got["labels"]), one["labels"]), what
    idx = _np(got["indices"])
    assert idx.dtype == np.int32
    if negative:
        assert np.array_equal(idx, np.flatnonzero(one["labels"] == wm.WM_SAC_OUTLIER)), what
    else:
        assert np.array_equal(idx, one["indices"]) and got["n_out"] == one["n_out"], what
    assert got["n_out"] == len(idx)


def _same_checker(wm, got, ref, what):
    assert got["rc"] == (wm.WM_OK if ref["status"] == SR.OK else wm.WM_NOT_CONVERGED), what
    for f in LOOP:
        assert got[f] == ref[f], (what, f, got[f], ref[f])
    if ref["status"] == SR.OK:
        assert got["refined"] == 0 and got["model_coefficients"].tobytes() == ref["model_coefficients"].tobytes(), what
        assert got["coefficients"].tobytes() == ref["model_coefficients"].tobytes(), what
        assert np.array_equal(_np(got["indices"]), ref["indices"]) and np.array_equal(_np(got["labels"]), ref["labels"]), what


def _case_of(name, kw):
    for i, (nm, thr, max_it, extra) in enumerate(SR.CASES):
        if nm == name and thr == kw["distance_threshold"] and max_it == kw["max_iterations"] and \
                extra.get("model", SR.PLANE) == kw.get("model", SR.PLANE):
            return i
    return None


def _against_singles(wm, ctx, names, kw, what, clouds=None, **more):
    shapes = SR.shapes()
    clouds = [shapes[n] for n in names] if clouds is None else clouds
    batch = ctx.sac_segment_batch(clouds, **kw, **more)
    assert len(batch) == len(clouds)
    singles = [_single(ctx, n, c, **kw) for n, c in zip(names, clouds)]
    for k, (g, s) in enumerate(zip(batch, singles)):
        assert g["batch_rc"] == wm.WM_OK
        _same(wm, g, s, "%s scan %d (%s)" % (what, k, names[k]), negative=bool(more.get("negative")))
    return batch, singles


# ------------------------------------------------------------------ 1. groups of the checker's cases
@pytest.mark.parametrize("optimize", [0, 1])
@pytest.mark.parametrize("group", ["A", "B", "decks", "decks+slab", "perp", "par50", "par200"])
def test_groups_of_the_checkers_cases(wm, ctx, group, optimize):
    names, kw = {"A": (GROUP_A, A), "B": (GROUP_B, B), "decks": (("decks",), dict(distance_threshold=0.25, max_iterations=50)),
                 "decks+slab": (("decks", "slab"), dict(distance_threshold=0.25, max_iterations=50)),
                 "perp": (("noisy_plane", "scene", "shell"), dict(A, **PERP)),
                 "par50": (("noisy_plane", "scene", "shell"), dict(A, **PAR)),
                 "par200": (("noisy_plane", "scene", "shell"), dict(A, max_iterations=200, **PAR))}[group]
    kw = dict(kw, optimize_coefficients=optimize)
    batch, singles = _against_singles(wm, ctx, names, kw, "group %s optimize %d" % (group, optimize))
    for name, g in zip(names, batch):
        print("%s %s: rc %d, %d iterations, %d skipped, %d entries in %d rounds, best entry %d with %d inliers, %d returned"
              % (group, name, g["rc"], g["iterations"], g["skipped"], g["hypotheses"], g["rounds"], g["best_hypothesis"],
                 g["n_inliers_model"], g["n_out"]))
        i = _case_of(name, kw)
        if i is not None and not optimize:
            _same_checker(wm, g, SR.case(i, optimize=False), "%s %s against the checker" % (group, name))
    by = dict(zip(names, batch))
    if group == "A":  # two scans end without a model (500 skipped each); a UTM scan stands beside scans at the origin
        for n in ("line", "point"):
            assert (by[n]["rc"], by[n]["skipped"], by[n]["iterations"]) == (wm.WM_NOT_CONVERGED, 500, 0)
        assert by["utm_plane"]["rc"] == wm.WM_OK and abs(by["utm_plane"]["coefficients"][3]) > 100
    if group == "B":  # the scans leave the batch in different rounds
        assert [by[n]["hypotheses"] for n in ("lattice", "dups", "shell", "line")] == [658, 921, 1001, 10000]
        assert [by[n]["rounds"] for n in ("lattice", "dups", "shell")] == [3, 4, 4] and by["line"]["rounds"] == 40
        assert by["point"]["rounds"] == 40 and by["line"]["rc"] == wm.WM_NOT_CONVERGED
    if group == "par50":
        assert by["scene"]["rc"] == wm.WM_NOT_CONVERGED and by["scene"]["iterations"] == 51


# ------------------------------------------------------------------ 2. company and order
def test_company_and_order_change_no_byte(wm, ctx):
    shapes = SR.shapes()
    perm = [int(v) for v in np.random.default_rng(3).permutation(len(GROUP_A))]
    for order in (list(range(len(GROUP_A)))[::-1], perm):
        names = [GROUP_A[i] for i in order]
        _against_singles(wm, ctx, names, A, "order %s" % order)
    for name in ("scene", "line"):
        _against_singles(wm, ctx, [name], A, "alone")
    a = ctx.sac_segment_batch([shapes[n] for n in GROUP_A], **A)
    b = ctx.sac_segment_batch([shapes[n] for n in GROUP_A], **A)
    for x, y in zip(a, b):
        _same(wm, x, y, "two calls")
    # the same cloud four times: no count may leak across scans
    four, _ = _against_singles(wm, ctx, ["scene"] * 4, A, "four times")
    for g in four[1:]:
        _same(wm, g, four[0], "four times")


# ------------------------------------------------------------------ 3. scan boundaries
def test_scan_boundaries(wm, ctx):
    import torch
    from libwave_amd import synth
    big = synth.scene(5000, seed=4)
    sizes = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097]
    clouds, names, at = [], [], 0
    for n in sizes:
        clouds.append(np.ascontiguousarray(big[at % 700:at % 700 + n]))
        names.append("scene5000[%d:+%d]" % (at % 700, n))
        at += 131
    nans = np.full((300, 3), np.nan, np.float32)
    three = nans.copy()
    three[[5, 150, 299]] = big[[1, 2, 3]]
    clouds += [nans, three]
    names += ["nan300", "three-finite"]
    for dev in (False, True):
        arrs = [torch.from_numpy(c.copy()).cuda() for c in clouds] if dev else clouds
        batch, singles = _against_singles(wm, ctx, names, A, "boundaries device %s" % dev, clouds=arrs)
        by = dict(zip(names, batch))
        for g, n in zip(batch[:3], sizes[:3]):  # n < 3: no sample
            assert g["rc"] == wm.WM_NOT_CONVERGED and g["n_out"] == 0 and g["hypotheses"] == 0 and g["rounds"] == 0
        g3 = batch[3]
        assert g3["rc"] == wm.WM_OK and g3["n_inliers_model"] == 3 and g3["refined"] == 0 and g3["n_out"] == 3
        assert by["nan300"]["rc"] == wm.WM_NOT_CONVERGED and by["nan300"]["n_finite"] == 0 and by["nan300"]["skipped"] == 500
        assert by["three-finite"]["n_finite"] == 3
        for g, c in zip(batch[4:len(sizes)], clouds[4:len(sizes)]):
            assert g["rc"] == wm.WM_OK and g["n_finite"] == len(c)


# ------------------------------------------------------------------ 4. the bins wrap
def test_a_scan_of_more_than_256_waves_between_small_ones(wm, ctx):
    scene = SR.shapes()["scene"]
    rng = np.random.default_rng(17)
    big = np.ascontiguousarray(np.tile(scene, (7, 1)) + rng.uniform(-1e-3, 1e-3, (7 * len(scene), 3)), np.float32)
    assert len(big) > 16384 + 64
    clouds = [np.ascontiguousarray(scene[:1000]), big, np.ascontiguousarray(scene[2000:2300])]
    names = ["scene[:1000]", "scene x 7", "scene[2000:2300]"]
    batch, singles = _against_singles(wm, ctx, names, A, "the bins wrap", clouds=clouds)
    assert all(g["refined"] == 1 for g in batch)
    assert batch[1]["coefficients"].tobytes() == singles[1]["coefficients"].tobytes()
    assert batch[1]["coefficients"].tobytes() != batch[1]["model_coefficients"].tobytes()
    _against_singles(wm, ctx, names[::-1], A, "the bins wrap, reversed", clouds=clouds[::-1])


# ------------------------------------------------------------------ 5. negative
def test_negative_hands_on_everything_but_the_plane(wm, ctx):
    import torch
    shapes = SR.shapes()
    names = ["scene", "line", "holes", "clumps_outliers"]
    clouds = [shapes[n] for n in names]
    plain = ctx.sac_segment_batch(clouds, **A)
    for dev in (False, True):
        arrs = [torch.from_numpy(c.copy()).cuda() for c in clouds] if dev else clouds
        kw = dict(A, negative=True)
        singles = [_single(ctx, n, c, **A) for n, c in zip(names, clouds)]
        batch, kept, offs = ctx.sac_segment_batch(arrs, points=True, **kw)
        for k, (g, s, p) in enumerate(zip(batch, singles, plain)):
            _same(wm, g, s, "negative %s" % names[k], negative=True)
            assert g["n_inliers"] == p["n_inliers"] == s["n_inliers"]  # (the inliers' number with either setting)
            want = np.flatnonzero(s["labels"] == wm.WM_SAC_OUTLIER) if s["rc"] == wm.WM_OK else np.zeros(0, np.int64)
            assert offs[k + 1] - offs[k] == len(want)
            assert _np(kept[offs[k]:offs[k + 1]]).tobytes() == clouds[k][want].tobytes(), names[k]
        assert batch[1]["rc"] == wm.WM_NOT_CONVERGED and offs[2] == offs[1]  # no model: nothing, with either setting
        assert batch[2]["n_out"] == batch[2]["n_finite"] - batch[2]["n_inliers"]  # (the holes are in neither list)
    # the device slices go into cluster_extract_batch as they are
    arrs = [torch.from_numpy(c.copy()).cuda() for c in clouds]
    batch, kept, offs = ctx.sac_segment_batch(arrs, points=True, negative=True, **A)
    assert kept.is_cuda
    rest_dev = [kept[offs[k]:offs[k + 1]] for k in range(len(clouds))]
    rest_host = [np.ascontiguousarray(clouds[k][_np(batch[k]["indices"])]) for k in range(len(clouds))]
    a = ctx.cluster_extract_batch(rest_dev, tolerance=0.5, min_cluster_size=5)
    b = ctx.cluster_extract_batch(rest_host, tolerance=0.5, min_cluster_size=5)
    assert sum(x["n_clusters"] for x in a) > 1
    for x, y in zip(a, b):
        assert x["n_clusters"] == y["n_clusters"]
        for f in ("labels", "indices", "offsets"):
            assert _np(x[f]).tobytes() == _np(y[f]).tobytes(), f


# ------------------------------------------------------------------ 6. memory and capacities
def _raw(wm, ctx, clouds, kw, cap, negative=0, out_stride=0, labels=True, stats=True, dev=False):
    """The C ABI on rows of any stride -> (rc, offsets, indices (cap + 4, filled with -7), points bytes, labels, status, coef)"""
    import torch
    S = len(clouds)
    stride = clouds[0].shape[1] * 4
    p = wm.sac_params(kw)
    keep = [torch.from_numpy(c.copy()).cuda() for c in clouds] if dev else clouds
    tab = (wm.SacScan * S)()
    for k, c in enumerate(keep):
        tab[k].pts, tab[k].n = (c.data_ptr() if dev else c.ctypes.data), len(c)
    total = sum(len(c) for c in clouds)
    offs, status, st = (C.c_size_t * (S + 1))(), (C.c_int * S)(), (wm.SacStats * S)()
    coef, ms = (C.c_float * (4 * S))(), C.c_float(0)
    mem = wm.WM_MEM_DEVICE if dev else wm.WM_MEM_HOST
    if dev:
        idx = torch.full((cap + 4,), -7, dtype=torch.int32, device="cuda")
        pts = torch.full(((cap + 4) * max(out_stride, 4) // 4,), -7.0, dtype=torch.float32, device="cuda")
        lab = torch.full((max(total, 1),), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        addr = lambda a: C.c_void_p(a.data_ptr())
    else:
        idx = np.full(cap + 4, -7, np.int32)
        pts = np.full((cap + 4) * max(out_stride, 4) // 4, -7.0, np.float32)
        lab = np.full(max(total, 1), 9, np.uint8)
        addr = lambda a: C.c_void_p(a.ctypes.data)
    rc = wm.lib().wm_sac_segment_batch(ctx._h, tab, S, stride, mem, C.byref(p), negative, coef, addr(idx), cap,
                                       addr(pts) if out_stride else None, out_stride, mem, offs, addr(lab) if labels else None,
                                       status, st if stats else None, C.byref(ms))
    return (rc, [int(v) for v in offs], _np(idx), _np(pts), _np(lab)[:total], list(status),
            np.array(coef[:], np.float32).reshape(S, 4), st)


def test_memory_strides_and_null_outputs_give_the_same_bytes(wm, ctx):
    shapes = SR.shapes()
    names = ["holes", "scene", "point", "noisy_plane"]
    clouds = [shapes[n] for n in names]
    singles = [_single(ctx, n, c, **A) for n, c in zip(names, clouds)]
    want_idx = np.concatenate([s["indices"] for s in singles])
    want_off = [0] + [int(v) for v in np.cumsum([len(s["indices"]) for s in singles])]
    want_lab = np.concatenate([s["labels"] if s["labels"] is not None else np.zeros(len(c), np.uint8)
                               for s, c in zip(singles, clouds)])
    want_pts = np.concatenate([c[s["indices"]] for s, c in zip(singles, clouds)])
    total = sum(len(c) for c in clouds)
    for width in (3, 4, 8):
        wide = [np.ascontiguousarray(np.c_[c, np.full((len(c), width - 3), 7.0, np.float32)], np.float32) for c in clouds]
        for dev in (False, True):
            for out_stride in (12, 16, 32):
                for labels, stats in ((True, True), (False, False)):
                    if (labels, stats) == (False, False) and (width, out_stride) != (4, 16):
                        continue
                    what = "stride %d device %s out_stride %d labels %s" % (width * 4, dev, out_stride, labels)
                    rc, offs, idx, pts, lab, status, coef, st = _raw(wm, ctx, wide, A, total, out_stride=out_stride,
                                                                       labels=labels, stats=stats, dev=dev)
                    m = want_off[-1]
                    assert rc == wm.WM_OK and offs == want_off, what
                    assert np.array_equal(idx[:m], want_idx) and (idx[total:] == -7).all(), what
                    rec = pts.reshape(-1, out_stride // 4)[:m]
                    assert rec[:, :3].tobytes() == want_pts.tobytes() and (rec[:, 3:] == 0).all(), what
                    assert (pts.reshape(-1, out_stride // 4)[total:] == -7.0).all(), what
                    assert np.array_equal(lab, want_lab) if labels else (lab == 9).all(), what
                    assert status == [s["rc"] for s in singles], what
                    for k, s in enumerate(singles):
                        if s["rc"] == wm.WM_OK:
                            assert coef[k].tobytes() == s["coefficients"].tobytes(), what
                        if stats:
                            assert [getattr(st[k], f) for f in STATS] == [s[f] for f in STATS], what
    # the wrapper: host clouds with device outputs and the other way round
    import torch
    for arrs, out_mem in ((clouds, wm.WM_MEM_DEVICE), ([torch.from_numpy(c.copy()).cuda() for c in clouds], wm.WM_MEM_HOST)):
        got = ctx.sac_segment_batch(arrs, out_mem=out_mem, **A)
        assert (out_mem == wm.WM_MEM_DEVICE) == (not isinstance(got[0]["indices"], np.ndarray))
        for k, (g, s) in enumerate(zip(got, singles)):
            _same(wm, g, s, "out_mem %d scan %d" % (out_mem, k))


@pytest.mark.parametrize("dev", [False, True])
def test_a_capacity_one_short_and_a_batch_of_one(wm, ctx, dev):
    shapes = SR.shapes()
    names = ["scene", "clumps_outliers"]
    clouds = [shapes[n] for n in names]
    singles = [_single(ctx, n, c, **A) for n, c in zip(names, clouds)]
    want_idx = np.concatenate([s["indices"] for s in singles])
    want_pts = np.concatenate([c[s["indices"]] for s, c in zip(singles, clouds)])
    m = len(want_idx)
    want_off = [0, len(singles[0]["indices"]), m]
    rc, offs, idx, pts, lab, status, coef, st = _raw(wm, ctx, clouds, A, m, out_stride=12, dev=dev)
    assert rc == wm.WM_OK and offs == want_off and np.array_equal(idx[:m], want_idx) and (idx[m:] == -7).all()
    rc, offs, idx, pts, lab, status, coef, st = _raw(wm, ctx, clouds, A, m - 1, out_stride=12, dev=dev)
    assert rc == wm.WM_ERR_ARG and offs == want_off and status == [wm.WM_OK, wm.WM_OK]
    assert np.array_equal(idx[:m - 1], want_idx[:m - 1]) and (idx[m - 1:] == -7).all()
    assert pts[:3 * (m - 1)].tobytes() == want_pts[:m - 1].tobytes() and (pts[3 * (m - 1):] == -7.0).all()
    assert np.array_equal(lab, np.concatenate([s["labels"] for s in singles]))
    assert st[1].n_inliers == singles[1]["n_inliers"] and coef[1].tobytes() == singles[1]["coefficients"].tobytes()
    short = ctx.sac_segment_batch(clouds, cap=m - 1, **A)
    assert short[0]["batch_rc"] == wm.WM_ERR_ARG and short[1]["n_out"] == len(singles[1]["indices"])
    assert len(short[1]["indices"]) == len(singles[1]["indices"]) - 1
    # a batch of one is the single call
    import torch
    for name in ("holes", "line"):
        P = shapes[name]
        arr = torch.from_numpy(P.copy()).cuda() if dev else P
        for opt in (0, 1):
            _against_singles(wm, ctx, [name], dict(A, optimize_coefficients=opt), "a batch of one", clouds=[arr])
    rc, offs, idx, pts, lab, status, coef, st = _raw(wm, ctx, [shapes["holes"]], A, 10, out_stride=16, dev=dev)
    one = _single(ctx, "holes", shapes["holes"], **A)
    assert rc == wm.WM_ERR_ARG and offs == [0, one["n_out"]] and np.array_equal(idx[:10], one["indices"][:10])
    assert (idx[10:] == -7).all() and pts.reshape(-1, 4)[:10, :3].tobytes() == shapes["holes"][one["indices"][:10]].tobytes()


# ------------------------------------------------------------------ 7. sac_round
def test_the_round_size_changes_no_byte_but_rounds(wm, ctx):
    shapes = SR.shapes()
    clouds = [shapes[n] for n in GROUP_A]
    outs = []
    try:
        for R in (1, 7, 256, 1024):
            ctx.set_option("sac_round", R)
            batch = ctx.sac_segment_batch(clouds, **A)
            for name, c, g in zip(GROUP_A, clouds, batch):
                one = ctx.sac_segment(c, **A)  # (under the same option: rounds must match)
                _same(wm, g, one, "sac_round %d %s" % (R, name))
                assert g["rounds"] >= -(-g["hypotheses"] // R)
            outs.append(batch)
    finally:
        ctx.set_option("sac_round", 256)
    assert [g["rounds"] for g in outs[0]] == [g["hypotheses"] for g in outs[0]]  # a round of one entry
    for batch in outs[1:]:
        for g, h in zip(batch, outs[0]):
            _same(wm, dict(g, rounds=0), dict(h, rounds=0), "across sac_round")


# ------------------------------------------------------------------ 8. the context's other state
def test_state_is_not_touched(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    shapes = SR.shapes()
    third = shapes["clumps_outliers"]
    scans = [shapes["scene"], third, shapes["line"]]
    runs = []
    for with_batch in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)  # (the target's normals are cached on the context)
            nrm_a = c.estimate_normals(1, 10)
            o1 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            c1 = c.cluster_extract(third, tolerance=0.5)
            s1 = c.sac_segment(third, distance_threshold=0.05)
            knn_a = c.debug_knn(1, 10)
            if with_batch:
                got = c.sac_segment_batch(scans, **A)
                assert [g["rc"] for g in got] == [wm.WM_OK, wm.WM_OK, wm.WM_NOT_CONVERGED] and got[1]["n_inliers_model"] == 2986
                assert all(g["rc"] == wm.WM_OK for g in c.sac_segment_batch([tgt_cloud, ref_cloud], points=True, negative=True,
                                                                            distance_threshold=0.1, max_iterations=300)[0])
            knn_b = c.debug_knn(1, 10)
            s2 = c.sac_segment(third, distance_threshold=0.05)
            o2 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            c2 = c.cluster_extract(third, tolerance=0.5)
            nrm_b = c.estimate_normals(1, 10)
            b = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            assert knn_a[0].tobytes() == knn_b[0].tobytes() and knn_a[1].tobytes() == knn_b[1].tobytes()
            assert c.sizes() == (len(ref_cloud), len(tgt_cloud))
            for k in ("indices", "labels", "counts"):
                assert o1[k].tobytes() == o2[k].tobytes()
            for k in ("indices", "labels", "offsets"):
                assert c1[k].tobytes() == c2[k].tobytes()
            _same(wm, s2, s1, "a single call after a batch")
            assert nrm_a.tobytes() == nrm_b.tobytes()
            runs.append((a, b, o2, c2, s2))
        finally:
            c.close()
    (a1, b1, o1, c1, s1), (a2, b2, o2, c2, s2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]
    assert o1["indices"].tobytes() == o2["indices"].tobytes() and o1["counts"].tobytes() == o2["counts"].tobytes()
    assert c1["indices"].tobytes() == c2["indices"].tobytes() and c1["labels"].tobytes() == c2["labels"].tobytes()
    _same(wm, s1, s2, "with and without a batch")
