"""wm_cluster_extract_batch (libwave_amd/csrc/wm_cluster.hip): a queue of scans through one sequence of launches.
Every output byte of a scan is a function of that scan's input alone, so every comparison here is equality: with the
single call (wm_cluster_extract on the scan alone), and through it or directly with the checker
(tests/cluster_reference.py).  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import cluster_reference as CR
import knn_reference as KR

pytestmark = pytest.mark.gpu

STATS = ("n_finite", "n_components", "n_clusters", "n_clustered", "largest")
ARRAYS = ("labels", "indices", "offsets")
NAMES14 = KR.NAMES + sorted(CR.OWN)


def _np(d):
    """a result dict with its arrays on the host"""
    out = dict(d)
    for k in ARRAYS:
        if d[k] is not None and not isinstance(d[k], np.ndarray):
            out[k] = d[k].cpu().numpy()
            if k == "offsets":
                out[k] = out[k].view(np.uint32)
    return out


def _equal(got, ref, what):
    got, ref = _np(got), _np(ref)
    assert got["rc"] == ref["rc"], what
    assert got["n_clusters"] == ref["n_clusters"] and got["n_out"] == ref["n_out"], (what, got["n_clusters"], ref["n_clusters"])
    for k in STATS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ARRAYS:
        if ref[k] is None or got[k] is None:
            assert ref.get(k) is None and got[k] is None, (what, k)
            continue
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k)


def _against_singles(ctx, clouds, what, **kw):
    batch = ctx.cluster_extract_batch(clouds, **kw)
    assert len(batch) == len(clouds)
    for k, cloud in enumerate(clouds):
        _equal(batch[k], ctx.cluster_extract(cloud, **kw), "%s scan %d" % (what, k))
    return batch


# ------------------------------------------------------------------ 1. against the checker
@pytest.mark.parametrize("tol", CR.TOLERANCES)
def test_fourteen_shapes_in_one_batch_equal_the_checker(wm, ctx, tol):
    shapes = CR.shapes()
    clouds = [shapes[name] for name in NAMES14]
    batch = _against_singles(ctx, clouds, "tolerance %.9g" % tol, tolerance=tol)
    for name, got in zip(NAMES14, batch):
        ref = CR.brute_case(name, tol)
        assert got["rc"] == wm.WM_OK
        for k in STATS + ("n_out",):
            assert got[k] == ref[k], (name, tol, k)
        for k in ARRAYS:
            assert np.array_equal(got[k], ref[k]), (name, tol, k)


# ------------------------------------------------------------------ 2. scans do not leak into each other
def test_five_copies_in_the_same_space_and_a_copy_shifted_by_the_tolerance(wm, ctx):
    scene = CR.shapes()["scene"]
    one = ctx.cluster_extract(scene, tolerance=2.0)
    batch = ctx.cluster_extract_batch([scene, scene.copy(), scene, scene.copy(), scene], tolerance=2.0)
    for k, got in enumerate(batch):
        _equal(got, one, "copy %d" % k)
    rails = CR.shapes()["rails"]
    for tol in (0.25, 0.2500001):
        moved = (rails + np.float32([0, tol, 0])).astype(np.float32)
        a, b = _against_singles(ctx, [rails, moved], "rails and rails + tolerance", tolerance=tol)
        ref = CR.brute_case("rails", tol)
        assert a["n_clusters"] == ref["n_clusters"] and np.array_equal(a["indices"], ref["indices"])
        together = CR.components_brute(np.r_[rails, moved], tol)
        assert a["n_clusters"] + b["n_clusters"] >= together["n_clusters"]  # (one call over both would merge some)


# ------------------------------------------------------------------ 3. scan boundaries
def _boundary_scans():
    rng = np.random.default_rng(314)
    nans = np.full((40, 3), np.nan, np.float32)
    nans[::3, 1] = np.inf
    nans[1::3, 0] = 1.0
    sizes = [0, 1, None, 63, 64, 65, 3000, 0, 129, 2]
    scans = []
    for n in sizes:
        if n is None:
            scans.append(nans)
        elif n == 3000:
            scans.append(CR.shapes()["clumps_outliers"][:3000])
        else:
            scans.append(rng.uniform(-1, 1, (n, 3)).astype(np.float32))
    return scans


def test_scan_boundaries_orders_and_repeats(wm, ctx):
    scans = _boundary_scans()
    for tol in (0.3, 5.0):
        fwd = _against_singles(ctx, scans, "boundaries tolerance %g" % tol, tolerance=tol)
        for i in (0, 2, 7):
            assert fwd[i]["n_clusters"] == 0 and fwd[i]["n_out"] == 0 and fwd[i]["offsets"].tolist() == [0]
        assert (fwd[2]["labels"] == wm.WM_CLUSTER_NONE).all() and len(fwd[2]["labels"]) == 40
        rev = ctx.cluster_extract_batch(scans[::-1], tolerance=tol)
        again = ctx.cluster_extract_batch(scans, tolerance=tol)
        for k in range(len(scans)):
            _equal(rev[len(scans) - 1 - k], fwd[k], "reversed %d" % k)
            for a in ARRAYS:
                assert again[k][a].tobytes() == fwd[k][a].tobytes(), (k, a)
    # nothing but empty scans, and nothing but scans without a finite point
    got = ctx.cluster_extract_batch([scans[0], scans[7]], tolerance=0.5)
    assert [g["n_clusters"] for g in got] == [0, 0] and got[0]["offsets"].tolist() == [0]
    got = _against_singles(ctx, [scans[2], scans[2][:7]], "all NaN", tolerance=0.5)
    assert (got[1]["labels"] == wm.WM_CLUSTER_NONE).all()


# ------------------------------------------------------------------ 4. ties across scans
def test_equal_sizes_go_by_scan_first(wm, ctx):
    def blobs(sizes, seed):  # blobs 10 m apart, their rows interleaved: equal sizes meet in every order
        rng = np.random.default_rng(seed)
        rows = np.concatenate([rng.uniform(-0.2, 0.2, (s, 3)) + [10.0 * j, 0, 0] for j, s in enumerate(sizes)])
        return np.ascontiguousarray(rows[rng.permutation(len(rows))], np.float32)

    a, b = blobs([7, 7, 5, 7, 5, 1], 1), blobs([5, 7, 7, 1, 7, 9], 2)
    got = _against_singles(ctx, [a, b], "ties", tolerance=1.0)
    assert np.diff(got[0]["offsets"].astype(np.int64)).tolist() == [7, 7, 7, 5, 5, 1]
    assert np.diff(got[1]["offsets"].astype(np.int64)).tolist() == [9, 7, 7, 7, 5, 1]
    for g in got:  # equal sizes: by the smallest member, the members ascending
        off, idx = g["offsets"].astype(np.int64), g["indices"]
        sizes = np.diff(off)
        firsts = idx[off[:-1]]
        for j in range(len(sizes) - 1):
            assert sizes[j] > sizes[j + 1] or firsts[j] < firsts[j + 1]
        assert all((np.diff(idx[off[j]:off[j + 1]]) > 0).all() for j in range(len(sizes)))
    # the raw numbering: scan 0's clusters first
    lab = np.empty(len(a) + len(b), np.int32)
    idx = np.empty(len(a) + len(b), np.int32)
    off = np.empty(len(a) + len(b) + 1, np.uint32)
    tab = (wm.ClusterScan * 2)()
    tab[0].pts, tab[0].n, tab[1].pts, tab[1].n = a.ctypes.data, len(a), b.ctypes.data, len(b)
    first, m = (C.c_size_t * 3)(), C.c_size_t(0)
    p = wm.cluster_params(tolerance=1.0)
    rc = wm.lib().wm_cluster_extract_batch(ctx._h, tab, 2, 12, wm.WM_MEM_HOST, C.byref(p), C.c_void_p(lab.ctypes.data),
                                           C.c_void_p(idx.ctypes.data), len(idx), None, 0, C.c_void_p(off.ctypes.data),
                                           len(idx), wm.WM_MEM_HOST, first, C.byref(m), None, None)
    assert rc == wm.WM_OK and list(first) == [0, 6, 12] and m.value == len(a) + len(b)
    assert np.diff(off[:13].astype(np.int64)).tolist() == [7, 7, 7, 5, 5, 1, 9, 7, 7, 7, 5, 1]
    assert np.array_equal(lab[:len(a)], got[0]["labels"]) and np.array_equal(lab[len(a):], got[1]["labels"])
    assert np.array_equal(idx[:len(a)], got[0]["indices"]) and np.array_equal(idx[len(a):], got[1]["indices"])


# ------------------------------------------------------------------ 5. the size rule
@pytest.mark.parametrize("lo,hi", [(2, CR.INT_MAX), (20, 100), (30, 5)])
def test_size_rule(wm, ctx, lo, hi):
    shapes = CR.shapes()
    clouds = [shapes["scene"], shapes["shell"]]
    full = ctx.cluster_extract_batch(clouds, tolerance=0.5)
    got = _against_singles(ctx, clouds, "sizes %d ... %d" % (lo, hi), tolerance=0.5, min_cluster_size=lo, max_cluster_size=hi)
    for k, name in enumerate(("scene", "shell")):
        ref = CR.with_size_rule(CR.brute_case(name, 0.5), lo, hi)
        assert np.array_equal(got[k]["labels"] == wm.WM_CLUSTER_REJECTED, ref["labels"] == CR.REJECTED)
        assert np.array_equal(got[k]["labels"], ref["labels"]) and np.array_equal(got[k]["indices"], ref["indices"])
        assert got[k]["n_components"] == full[k]["n_components"] == ref["n_components"]
        if hi < lo:
            assert got[k]["n_clusters"] == 0 and got[k]["offsets"].tolist() == [0] and got[k]["largest"] == 0
            assert (got[k]["labels"] == wm.WM_CLUSTER_REJECTED).all()


# ------------------------------------------------------------------ 6. the cell rule
def test_the_cell_rule_changes_no_byte(wm, ctx):
    shapes = CR.shapes()
    names = ["lattice", "rails", "utm", "clumps_outliers"]
    clouds = [shapes[n] for n in names]
    try:
        for div in (0.5, 2.0, 8.0):
            ctx.set_option("cluster_cell_div", div)
            for tol in (0.05, 0.5):
                got = ctx.cluster_extract_batch(clouds, tolerance=tol)
                for name, g in zip(names, got):
                    ref = CR.brute_case(name, tol)
                    for k in ARRAYS:
                        assert np.array_equal(g[k], ref[k]), (name, div, tol, k)
                    assert [g[k] for k in STATS] == [ref[k] for k in STATS]
    finally:
        ctx.set_option("cluster_cell_div", 2.0)


# ------------------------------------------------------------------ 7. plumbing
def _raw(wm, ctx, arrays, stride, mem, out_mem, p, labels=True, out_stride=0, cap=None, cap_clusters=None, stats=True):
    """The C entry point with every output pre-filled -> (rc, first, n_out, labels, indices, points, offsets)."""
    import torch
    S, total = len(arrays), sum(len(a) for a in arrays)
    tab = (wm.ClusterScan * max(S, 1))()
    for k, a in enumerate(arrays):
        tab[k].pts = a.data_ptr() if mem == wm.WM_MEM_DEVICE else a.ctypes.data
        tab[k].n = len(a)
    cap = total if cap is None else cap
    cap_clusters = total if cap_clusters is None else cap_clusters
    lab = np.full(total, -7, np.int32)
    idx = np.full(cap + 1, -7, np.int32)
    off = np.full(cap_clusters + 2, 9, np.uint32)
    pts = np.full((cap + 1) * max(out_stride, 4), 0xAB, np.uint8)
    if out_mem == wm.WM_MEM_DEVICE:
        hold = [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda() for x in (lab, idx, off, pts)]
        torch.cuda.synchronize()
        ptrs = [h.data_ptr() for h in hold]
    else:
        hold = [lab, idx, off, pts]
        ptrs = [h.ctypes.data for h in hold]
    first, m = (C.c_size_t * (S + 1))(), C.c_size_t(0)
    st = (wm.ClusterStats * max(S, 1))()
    rc = wm.lib().wm_cluster_extract_batch(ctx._h, tab, S, stride, mem, C.byref(p), C.c_void_p(ptrs[0]) if labels else None,
                                           C.c_void_p(ptrs[1]), cap, C.c_void_p(ptrs[3]) if out_stride else None, out_stride,
                                           C.c_void_p(ptrs[2]), cap_clusters, out_mem, first, C.byref(m),
                                           st if stats else None, None)
    if out_mem == wm.WM_MEM_DEVICE:
        lab, idx, off, pts = [h.cpu().numpy() for h in hold]
        off = off.view(np.uint32)
    return rc, [int(v) for v in first], m.value, lab, idx, pts, off


def test_memories_strides_null_arrays_and_points_out(wm, ctx):
    import torch
    shapes = CR.shapes()
    clouds = [shapes["holes"], shapes["scene"], shapes["dups"]]
    sizes = [len(c) for c in clouds]
    total = sum(sizes)
    p = wm.cluster_params(tolerance=2.0, min_cluster_size=2)
    ones = [ctx.cluster_extract(c, tolerance=2.0, min_cluster_size=2) for c in clouds]
    want_lab = np.concatenate([o["labels"] for o in ones])
    want_idx = np.concatenate([o["indices"] for o in ones])
    want_first = np.r_[0, np.cumsum([o["n_clusters"] for o in ones])].tolist()
    base = np.r_[0, np.cumsum([o["n_out"] for o in ones])]
    want_off = np.concatenate([o["offsets"][:-1].astype(np.int64) + base[k] for k, o in enumerate(ones)] + [base[-1:]]).astype(np.uint32)
    want_xyz = np.concatenate([c[o["indices"]] for c, o in zip(clouds, ones)])
    kept, ncl = len(want_idx), want_first[-1]
    assert 1 < kept < total and ncl > 3

    def widen(c, cols):
        return np.ascontiguousarray(np.c_[c, np.full((len(c), cols - 3), 7.0, np.float32)], np.float32) if cols > 3 else c

    for stride in (12, 16, 32):
        host = [widen(c, stride // 4) for c in clouds]
        for mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
            arrays = host if mem == wm.WM_MEM_HOST else [torch.from_numpy(h.copy()).cuda() for h in host]
            for out_mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
                for out_stride in (0, 12, 16):
                    if out_stride and stride == 32 and mem != out_mem:
                        continue  # (enough combinations)
                    what = (stride, mem, out_mem, out_stride)
                    rc, first, m, lab, idx, pts, off = _raw(wm, ctx, arrays, stride, mem, out_mem, p, out_stride=out_stride)
                    assert rc == wm.WM_OK and first == want_first and m == kept, what
                    assert np.array_equal(lab, want_lab), what
                    assert np.array_equal(idx[:kept], want_idx) and (idx[kept:] == -7).all(), what
                    assert np.array_equal(off[:ncl + 1], want_off) and (off[ncl + 1:] == 9).all(), what
                    if out_stride:
                        rec = pts[:kept * out_stride].reshape(kept, out_stride)
                        assert rec[:, :12].tobytes() == want_xyz.tobytes(), what
                        assert not rec[:, 12:].any() and (pts[kept * out_stride:] == 0xAB).all(), what
    # labels_out = NULL and stats = NULL
    rc, first, m, lab, idx, pts, off = _raw(wm, ctx, clouds, 12, wm.WM_MEM_HOST, wm.WM_MEM_HOST, p, labels=False, stats=False)
    assert rc == wm.WM_OK and first == want_first and (lab == -7).all() and np.array_equal(idx[:kept], want_idx)
    got = ctx.cluster_extract_batch(clouds, labels=False, tolerance=2.0, min_cluster_size=2)
    assert all(g["labels"] is None for g in got) and np.array_equal(got[1]["indices"], ones[1]["indices"])
    # one index short: the prefixes, the offsets clamped to cap; one cluster short: cap_clusters + 1 offsets
    for out_mem in (wm.WM_MEM_HOST, wm.WM_MEM_DEVICE):
        rc, first, m, lab, idx, pts, off = _raw(wm, ctx, clouds, 12, wm.WM_MEM_HOST, out_mem, p, out_stride=16, cap=kept - 1)
        assert rc == wm.WM_ERR_ARG and first == want_first and m == kept
        assert np.array_equal(idx, np.r_[want_idx[:kept - 1], np.int32(-7)])
        assert pts[:(kept - 1) * 16].reshape(-1, 16)[:, :12].tobytes() == want_xyz[:kept - 1].tobytes()
        assert (pts[(kept - 1) * 16:kept * 16] == 0xAB).all()
        assert np.array_equal(off[:ncl + 1], np.minimum(want_off, kept - 1))
        rc, first, m, lab, idx, pts, off = _raw(wm, ctx, clouds, 12, wm.WM_MEM_HOST, out_mem, p, cap_clusters=ncl - 1)
        assert rc == wm.WM_ERR_ARG and first == want_first and m == kept
        assert np.array_equal(idx[:kept], want_idx)
        assert np.array_equal(off, np.r_[want_off[:ncl], np.uint32(9)])
    # the wrapper in device memory, points included
    dev = [torch.from_numpy(c.copy()).cuda() for c in clouds]
    got, pts_d, offs = ctx.cluster_extract_batch(dev, points=True, tolerance=2.0, min_cluster_size=2)
    assert pts_d.is_cuda and got[0]["indices"].is_cuda and offs.tolist() == base.tolist()
    assert pts_d.cpu().numpy().tobytes() == want_xyz.tobytes()
    for g, o in zip(got, ones):
        _equal(g, o, "device wrapper")


# ------------------------------------------------------------------ 8. size
def test_eight_slices_of_the_large_scene(wm, ctx):
    """The batch is past the 256k switch between rocPRIM and rs_sort_pairs; no scan is."""
    cloud = CR.big_cloud()
    edges = np.linspace(0, len(cloud), 9).astype(int)
    slices = [np.ascontiguousarray(cloud[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    assert len(cloud) > 256 << 10 and max(len(s) for s in slices) < 256 << 10
    for tol in CR.BIG_TOLERANCES:
        got = _against_singles(ctx, slices, "big tolerance %g" % tol, tolerance=tol)
        ref = CR.components(slices[3], tol)
        for k in ARRAYS:
            assert np.array_equal(got[3][k], ref[k]), (tol, k)
        assert [got[3][k] for k in STATS] == [ref[k] for k in STATS]


# ------------------------------------------------------------------ 9. the context
def test_state_is_not_touched_and_the_workspace_is_shared(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    shapes = CR.shapes()
    third = shapes["clumps_outliers"]
    queue = [third, shapes["scene"], tgt_cloud]
    runs = []
    for with_batch in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            o1 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            n1 = c.estimate_normals(1)
            if with_batch:
                before = c.cluster_extract(third, tolerance=0.5)
                got = c.cluster_extract_batch(queue, tolerance=0.5)
                after = c.cluster_extract(third, tolerance=0.5)  # a single call behind a batch, and the other way round
                _equal(after, before, "single after batch")
                _equal(got[0], before, "batch after single")
                assert before["n_clusters"] == 14
                again = c.cluster_extract_batch(queue[::-1], tolerance=0.5)
                for k in range(3):
                    _equal(again[2 - k], got[k], "batch after single after batch")
            n2 = c.estimate_normals(1)
            o2 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            b = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            assert n1.tobytes() == n2.tobytes() and c.sizes() == (len(ref_cloud), len(tgt_cloud))
            for k in ("indices", "labels", "counts"):
                assert o1[k].tobytes() == o2[k].tobytes()
            runs.append((a, b, o2, n2))
        finally:
            c.close()
    (a1, b1, o1, n1), (a2, b2, o2, n2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]
    assert o1["indices"].tobytes() == o2["indices"].tobytes() and n1.tobytes() == n2.tobytes()


# ------------------------------------------------------------------ 10. the pipeline in device memory
def test_ground_batch_into_cluster_batch_into_icp_batch(wm, ctx):
    import torch
    import ground_scenes as S
    scans = [torch.from_numpy(S.rings_sensor_frame(20_000, seed=42 + k)).cuda() for k in range(4)]
    _, kept, goff = ctx.ground_segment_batch(scans, points=True)
    assert kept.is_cuda
    slices = [kept[goff[k]:goff[k + 1]] for k in range(4)]
    assert min(len(s) for s in slices) > 500
    got, pts, poff = ctx.cluster_extract_batch(slices, points=True, tolerance=0.5, min_cluster_size=20)
    assert pts.is_cuda and pts.shape[1] == kept.shape[1]
    hosts = []
    for k in range(4):
        _equal(got[k], ctx.cluster_extract(slices[k], tolerance=0.5, min_cluster_size=20), "obstacles of scan %d" % k)
        host = slices[k].cpu().numpy()
        idx = got[k]["indices"].cpu().numpy()
        assert len(idx) > 100 and (got[k]["labels"].cpu().numpy() == wm.WM_CLUSTER_REJECTED).any()
        rows = np.zeros((len(idx), pts.shape[1]), np.float32)  # (gathered on the host: x y z, the rest zero)
        rows[:, :3] = host[idx][:, :3]
        assert pts[poff[k]:poff[k + 1]].cpu().numpy().tobytes() == rows.tobytes()
        hosts.append(torch.from_numpy(rows).cuda())
    # each scan's clustered points registered against themselves moved a little: the device slices as they are, and
    # the same points gathered on the host
    c, sn = np.cos(0.02), np.sin(0.02)
    R = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]])
    targets = []
    for k in range(4):
        rows = hosts[k].cpu().numpy().copy()
        rows[:, :3] = (rows[:, :3].astype(np.float64) @ R.T + [0.3, -0.1, 0.02]).astype(np.float32)
        targets.append(torch.from_numpy(rows).cuda())
    on_device = [(pts[poff[k]:poff[k + 1]], targets[k]) for k in range(4)]
    gathered = [(hosts[k], targets[k]) for k in range(4)]
    ra = ctx.icp_batch_match(on_device, with_info=False, max_corr=3.0)
    rb = ctx.icp_batch_match(gathered, with_info=False, max_corr=3.0)
    for x, y in zip(ra, rb):
        assert x["rc"] == y["rc"] == wm.WM_OK and x["T"].tobytes() == y["T"].tobytes()
        assert x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"] > 100
