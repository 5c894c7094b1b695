"""wm_sac_segment (libwave_amd/csrc/wm_sac.hip) on the GPU against tests/sac_reference.py.

The loop is compared EXACTLY on every case of the checker: status, iterations, skipped, hypotheses, best_hypothesis,
n_inliers_model and the bits of the model's coefficients -- and, without the refit, the indices, the labels and the
bits of the returned coefficients.  With the refit the indices and labels must equal the checker's selection FROM THE
RETURNED coefficients, and the coefficients are held to the checker's float64 eigh (C the covariance of the model's
inliers, l0 <= l1 <= l2 its eigenvalues):
    n' C n <= l0 (1 + 1e-9) + 1e-12 l2        rounding a unit vector to float turns it by <= 2^-23, whose square is
                                              1.4e-14: two orders of margin.  (The refit rounds the normal TOWARD ZERO,
                                              so n is never longer than 1: a vector rounded to nearest can be longer by
                                              3e-8, which alone adds 6e-8 l0 -- more than the bound where l0 is large,
                                              e.g. 1.1e-9 against 8.8e-10 on `scene` at 0.5.)
    | |n| - 1 | <= 4 * 2^-23
    | d + n . centroid | <= 4 ulp32(max(1, |d|))
    n . (the model's normal) > 0
    where l1 >= 100 l0 > 0: every component within 4 * 2^-23 of the checker's
tests/test_sac_reference_cpu.py holds the checker's two forms to each other on every case used here."""
import ctypes as C

import numpy as np
import pytest

import sac_reference as SR

pytestmark = pytest.mark.gpu

LOOP = ("iterations", "skipped", "hypotheses", "best_hypothesis", "n_inliers_model")
U = 2.0 ** -23


def _kw(thr, max_it, extra, **more):
    kw = dict(distance_threshold=thr, max_iterations=max_it)
    for k, v in extra.items():
        kw[{"prob": "probability"}.get(k, k)] = v
    kw.update(more)
    return kw


def _host(got):
    out = dict(got)
    for k in ("indices", "labels"):
        if out[k] is not None and not isinstance(out[k], np.ndarray):
            out[k] = out[k].cpu().numpy()
    return out


def _same_loop(wm, got, ref, what):
    print("%s: rc %d, %d iterations, %d skipped, %d entries in %d rounds, best entry %d with %d inliers; %.3f ms on the "
          "device" % (what, got["rc"], got["iterations"], got["skipped"], got["hypotheses"], got["rounds"],
                      got["best_hypothesis"], got["n_inliers_model"], got["kernel_ms"]))
    assert got["rc"] == (wm.WM_OK if ref["status"] == SR.OK else wm.WM_NOT_CONVERGED), what
    for k in LOOP:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    if ref["status"] == SR.OK:
        assert got["model_coefficients"].tobytes() == ref["model_coefficients"].tobytes(), what
    else:
        assert got["n_out"] == 0 and len(got["indices"]) == 0 and got["coefficients"] is None, what


def _same_unrefined(got, ref, what):
    assert got["refined"] == 0 and got["coefficients"].tobytes() == ref["model_coefficients"].tobytes(), what
    assert got["indices"].dtype == np.int32 and np.array_equal(got["indices"], ref["indices"]), what
    assert got["labels"].dtype == np.uint8 and np.array_equal(got["labels"], ref["labels"]), what
    assert got["n_out"] == got["n_inliers"] == got["n_inliers_model"] == len(ref["indices"]), what


def _refit_ok(P, got, thr, what, close=None):
    """the returned coefficients against the checker's float64 plane of the model's inliers; -> whether l1 >= 100 l0 > 0"""
    coef = got["coefficients"]
    idx, lab = SR.select(P, coef, thr)
    assert np.array_equal(got["indices"], idx) and np.array_equal(got["labels"], lab), what
    assert got["n_out"] == got["n_inliers"] == len(idx), what
    if got["n_inliers_model"] < 4:
        assert got["refined"] == 0 and coef.tobytes() == got["model_coefficients"].tobytes(), what
        return False
    assert got["refined"] == 1, what
    f = SR.refit(P, got["model_coefficients"], thr)
    l0, l1, l2 = f["lam"]
    n, d = coef[:3].astype(np.float64), float(coef[3])
    ray, norm = n @ f["C"] @ n, np.linalg.norm(n)
    gap = l1 >= 100 * l0 and l0 > 0
    print("%s: eigenvalues %.3g %.3g %.3g; n'Cn - l0 = %.3g (allowed %.3g), |n| - 1 = %.3g, d + n.c = %.3g (allowed %.3g), "
          "largest component difference %.3g%s"
          % (what, l0, l1, l2, ray - l0, l0 * 1e-9 + 1e-12 * l2, norm - 1, d + n @ f["centroid"],
             4 * float(np.spacing(np.float32(max(1.0, abs(d))))), np.abs(n - f["n"]).max(), " (held)" if gap else ""))
    assert ray <= l0 * (1 + 1e-9) + 1e-12 * l2, (what, ray, l0, l2)
    assert abs(norm - 1) <= 4 * U, (what, norm)
    assert abs(d + n @ f["centroid"]) <= 4 * float(np.spacing(np.float32(max(1.0, abs(d))))), (what, d, n @ f["centroid"])
    assert n @ got["model_coefficients"][:3].astype(np.float64) > 0, what
    if gap:
        assert np.abs(n - f["n"]).max() <= 4 * U, (what, n, f["n"])
    if close is not None:
        assert gap == close, (what, f["lam"])
    return gap


# ------------------------------------------------------------------ against the checker
@pytest.mark.parametrize("i", range(len(SR.CASES)), ids=SR.case_id)
def test_equals_the_checker(wm, ctx, i):
    name, thr, max_it, extra = SR.CASES[i]
    P = SR.shapes()[name]
    ref = SR.case(i, optimize=False)
    got = ctx.sac_segment(P, **_kw(thr, max_it, extra, optimize_coefficients=0))
    _same_loop(wm, got, ref, SR.case_id(i) + " without the refit")
    assert got["n_finite"] == np.isfinite(P).all(1).sum()
    if ref["status"] == SR.OK:
        _same_unrefined(got, ref, SR.case_id(i))
    got = ctx.sac_segment(P, **_kw(thr, max_it, extra))
    _same_loop(wm, got, ref, SR.case_id(i))
    if ref["status"] == SR.OK:
        close = True if name in ("scene", "holes", "noisy_plane", "utm_plane") and not extra and thr == 0.05 else None
        _refit_ok(P, got, thr, SR.case_id(i), close=close)
    if name == "holes":
        holes = [0, 17, 1500, len(P) - 1]
        assert got["n_finite"] == 2996 and (got["labels"][holes] == wm.WM_SAC_NONE).all()
        assert not np.isin(holes, got["indices"]).any()
    if name == "decks":  # strict: the plane z = 0 would take its own layer only; the stream finds a tilted one
        assert got["n_inliers_model"] == 1450


def test_utm_plane_refit_at_large_offsets(wm, ctx):
    """the refit's sums are relative to the sample's p0: the plane at 1e5 m is the plane at the origin, moved"""
    near, far = SR.shapes()["noisy_plane"], SR.shapes()["utm_plane"]
    a = ctx.sac_segment(near, distance_threshold=0.05)
    b = ctx.sac_segment(far, distance_threshold=0.05)
    assert _refit_ok(near, a, 0.05, "noisy_plane") and _refit_ok(far, b, 0.05, "utm_plane")
    assert b["n_inliers_model"] == 2999 and abs(b["coefficients"][3]) > 100
    ang = np.arccos(min(1.0, float(a["coefficients"][:3].astype(np.float64) @ b["coefficients"][:3].astype(np.float64))))
    assert ang < 1e-3, ang  # (the float coordinates at 1e5 m are rounded to 8 mm: the same plane up to that)


# ------------------------------------------------------------------ rounds, repeatability
@pytest.mark.parametrize("name", ["lattice", "dups"])
def test_the_round_size_changes_no_byte(wm, ctx, name):
    P = SR.shapes()[name]
    i = [c[0] for c in SR.CASES].index(name)
    ref = SR.case(i)
    outs = []
    try:
        for R in (1, 7, 256, 1024):
            ctx.set_option("sac_round", R)
            got = ctx.sac_segment(P, distance_threshold=0.5, max_iterations=1000)
            _same_loop(wm, got, ref, "%s sac_round %d" % (name, R))
            assert got["rounds"] >= -(-got["hypotheses"] // R)
            outs.append(got)
    finally:
        ctx.set_option("sac_round", 256)
    for got in outs[1:]:
        for k in ("coefficients", "indices", "labels", "model_coefficients"):
            assert got[k].tobytes() == outs[0][k].tobytes(), (name, k)
        assert got["n_out"] == outs[0]["n_out"] and got["refined"] == outs[0]["refined"]
    for bad in (0, 1025):
        with pytest.raises(wm.WmError):
            ctx.set_option("sac_round", bad)


def test_two_calls_give_identical_bytes(wm, ctx):
    for name, thr in (("scene", 0.05), ("clumps_outliers", 0.05), ("shell", 0.5)):
        P = SR.shapes()[name]
        a = ctx.sac_segment(P, distance_threshold=thr, max_iterations=100)
        b = ctx.sac_segment(P, distance_threshold=thr, max_iterations=100)
        for k in ("coefficients", "indices", "labels", "model_coefficients"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        assert [a[k] for k in LOOP] == [b[k] for k in LOOP]
    c = ctx.sac_segment(SR.shapes()["scene"], distance_threshold=0.05, max_iterations=100, seed=12345)
    ref = SR.segment(SR.shapes()["scene"], 0.05, max_it=100, seed=12345)  # (a seed moves the stream)
    _same_loop(wm, c, ref, "scene seed 12345")


def test_a_row_permutation_keeps_the_invariants(wm, ctx):
    """another order is another stream: the checker is run on the permuted array, and the inliers are near the plane"""
    P = SR.shapes()["scene"]
    perm = np.random.default_rng(5).permutation(len(P))
    Q = np.ascontiguousarray(P[perm])
    ref = SR.segment(Q, 0.05, optimize=False)
    got = ctx.sac_segment(Q, distance_threshold=0.05, optimize_coefficients=0)
    _same_loop(wm, got, ref, "scene permuted")
    _same_unrefined(got, ref, "scene permuted")
    got = ctx.sac_segment(Q, distance_threshold=0.05)
    _refit_ok(Q, got, 0.05, "scene permuted")
    c = got["coefficients"].astype(np.float64)
    dist = np.abs(Q[got["indices"]].astype(np.float64) @ c[:3] + c[3])
    assert (dist < 0.05 * (1 + 1e-5) + 1e-5).all() and got["n_out"] > 1000


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65])
def test_tiny_clouds(wm, ctx, n):
    rng = np.random.default_rng(100 + n)
    P = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    P[:, 2] *= 0.05
    for thr in (0.02, 5.0):
        ref = SR.segment(P, thr, optimize=False)
        got = ctx.sac_segment(P, distance_threshold=thr, optimize_coefficients=0)
        _same_loop(wm, got, ref, "n %d threshold %g" % (n, thr))
        if n < 3:
            assert got["rc"] == wm.WM_NOT_CONVERGED and got["hypotheses"] == 0 and got["rounds"] == 0
            continue
        _same_unrefined(got, ref, "n %d" % n)
        _refit_ok(P, ctx.sac_segment(P, distance_threshold=thr), thr, "n %d threshold %g" % (n, thr))


def test_all_nan_clouds_have_no_model(wm, ctx):
    import torch
    nans = np.full((100, 3), np.nan, np.float32)
    nans[::3, 1] = np.inf
    nans[1::3, 0] = 1.0  # (x finite, y not)
    for arr in (nans, torch.from_numpy(nans.copy()).cuda()):
        got = ctx.sac_segment(arr, distance_threshold=0.5, max_iterations=5)
        assert got["rc"] == wm.WM_NOT_CONVERGED and got["n_out"] == 0 and got["n_finite"] == 0
        assert (got["iterations"], got["skipped"], got["hypotheses"], got["best_hypothesis"]) == (0, 50, 50, -1)


def test_large_scene_against_the_checker(wm, ctx):
    """270 000 points: 264 tiles of the count kernel, more than one workgroup per plane"""
    from libwave_amd import synth
    P = synth.scene(270000, seed=9)
    ref = SR.segment(P, 0.05, optimize=False, block=64)
    got = ctx.sac_segment(P, distance_threshold=0.05, optimize_coefficients=0)
    _same_loop(wm, got, ref, "scene(270000)")
    _same_unrefined(got, ref, "scene(270000)")
    _refit_ok(P, ctx.sac_segment(P, distance_threshold=0.05), 0.05, "scene(270000)")


# ------------------------------------------------------------------ plumbing
def test_host_and_device_memory_and_strides_give_the_same_bytes(wm, ctx):
    import torch
    P = SR.shapes()["holes"]
    first = ctx.sac_segment(P, distance_threshold=0.05)
    _refit_ok(P, first, 0.05, "holes")
    c4 = np.c_[P, np.full(len(P), 7.0, np.float32)].astype(np.float32)
    c8 = np.ascontiguousarray(np.c_[c4, c4], np.float32)
    for host in (P, c4):
        for arr in (host, torch.from_numpy(host.copy()).cuda()):
            for out_mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
                got = ctx.sac_segment(arr, distance_threshold=0.05, out_mem=out_mem)
                if out_mem == wm.WM_MEM_DEVICE:
                    assert got["indices"].is_cuda and got["labels"].is_cuda
                got = _host(got)
                for k in ("coefficients", "indices", "labels", "model_coefficients"):
                    assert got[k].tobytes() == first[k].tobytes(), (k, host.shape, type(arr), out_mem)
                assert [got[k] for k in LOOP] == [first[k] for k in LOOP] and got["n_finite"] == first["n_finite"]
    # stride 32 through the C ABI
    n = len(P)
    p = wm.sac_params(distance_threshold=0.05)
    idx, lab, coef = np.empty(n, np.int32), np.empty(n, np.uint8), (C.c_float * 4)()
    m = C.c_size_t(0)
    rc = wm.lib().wm_sac_segment(ctx._h, C.c_void_p(c8.ctypes.data), n, 32, wm.WM_MEM_HOST, C.byref(p), coef,
                                 C.c_void_p(idx.ctypes.data), n, wm.WM_MEM_HOST, C.byref(m), C.c_void_p(lab.ctypes.data), None)
    assert rc == wm.WM_OK and m.value == first["n_out"]
    assert np.array(coef[:], np.float32).tobytes() == first["coefficients"].tobytes()
    assert np.array_equal(idx[:m.value], first["indices"]) and np.array_equal(lab, first["labels"])


def test_labels_out_may_be_null(wm, ctx):
    P = SR.shapes()["scene"]
    full = ctx.sac_segment(P, distance_threshold=0.05)
    got = ctx.sac_segment(P, distance_threshold=0.05, labels=False)
    assert got["rc"] == wm.WM_OK and got["labels"] is None
    assert np.array_equal(got["indices"], full["indices"]) and got["coefficients"].tobytes() == full["coefficients"].tobytes()


@pytest.mark.parametrize("device", [False, True])
def test_a_capacity_one_short_is_an_argument_error_with_the_true_count(wm, ctx, device):
    import torch
    P = SR.shapes()["scene"]
    src = torch.from_numpy(P.copy()).cuda() if device else P
    full = _host(ctx.sac_segment(src, distance_threshold=0.05))
    m = full["n_out"]
    assert full["rc"] == wm.WM_OK and 1 < m < len(P)
    exact = _host(ctx.sac_segment(src, distance_threshold=0.05, cap=m))
    assert exact["rc"] == wm.WM_OK and np.array_equal(exact["indices"], full["indices"])
    short = _host(ctx.sac_segment(src, distance_threshold=0.05, cap=m - 1))
    assert short["rc"] == wm.WM_ERR_ARG and short["n_out"] == m and len(short["indices"]) == m - 1
    assert np.array_equal(short["indices"], full["indices"][:m - 1])
    assert short["coefficients"].tobytes() == full["coefficients"].tobytes() and np.array_equal(short["labels"], full["labels"])
    none = _host(ctx.sac_segment(src, distance_threshold=0.05, cap=0))  # (indices_out may then be anything: nothing is written)
    assert none["rc"] == wm.WM_ERR_ARG and none["n_out"] == m and len(none["indices"]) == 0


# ------------------------------------------------------------------ the context's other state
def test_state_is_not_touched(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    third = SR.shapes()["clumps_outliers"]
    runs = []
    for with_sac in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)  # (the target's normals are cached on the context)
            o1 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            c1 = c.cluster_extract(third, tolerance=0.5)
            knn_a = c.debug_knn(1, 10)
            if with_sac:
                got = c.sac_segment(third, distance_threshold=0.05)
                assert got["rc"] == wm.WM_OK and got["n_inliers_model"] == 2986
                assert c.sac_segment(tgt_cloud, distance_threshold=0.1, max_iterations=300)["rc"] == wm.WM_OK
            knn_b = c.debug_knn(1, 10)
            o2 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            c2 = c.cluster_extract(third, tolerance=0.5)
            b = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            assert knn_a[0].tobytes() == knn_b[0].tobytes() and knn_a[1].tobytes() == knn_b[1].tobytes()
            assert c.sizes() == (len(ref_cloud), len(tgt_cloud))
            for k in ("indices", "labels", "counts"):
                assert o1[k].tobytes() == o2[k].tobytes()
            for k in ("indices", "labels", "offsets"):
                assert c1[k].tobytes() == c2[k].tobytes()
            runs.append((a, b, o2, c2))
        finally:
            c.close()
    (a1, b1, o1, c1), (a2, b2, o2, c2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]
    assert o1["indices"].tobytes() == o2["indices"].tobytes() and o1["counts"].tobytes() == o2["counts"].tobytes()
    assert c1["indices"].tobytes() == c2["indices"].tobytes() and c1["labels"].tobytes() == c2["labels"].tobytes()


# ------------------------------------------------------------------ the pipeline
def test_plane_off_then_clusters_on_the_device(wm, ctx, testscan):
    import torch
    import cluster_reference as CR
    host = np.ascontiguousarray(testscan[:, :3], np.float32)
    scan = torch.from_numpy(host).cuda()
    got = ctx.sac_segment(scan, distance_threshold=0.2, max_iterations=100)
    assert got["rc"] == wm.WM_OK and got["indices"].is_cuda and got["labels"].is_cuda
    ref = SR.segment(host, 0.2, optimize=False, max_it=100)
    _same_loop(wm, got, ref, "the scan")
    _refit_ok(host, _host(got), 0.2, "the scan")
    assert got["n_out"] > len(host) // 10
    rest = scan[got["labels"] == wm.WM_SAC_OUTLIER].contiguous()  # what is left when the plane is peeled off
    assert rest.is_cuda and len(rest) == got["n_finite"] - got["n_out"]
    cl = ctx.cluster_extract(rest, tolerance=0.5, min_cluster_size=10)
    assert cl["indices"].is_cuda
    want = CR.components(rest.cpu().numpy(), 0.5, min_cluster_size=10)
    assert cl["n_clusters"] == want["n_clusters"] > 1
    assert np.array_equal(cl["indices"].cpu().numpy(), want["indices"]) and np.array_equal(cl["labels"].cpu().numpy(), want["labels"])
