"""wm_cluster_boxes on the device against tests/boxes_reference.py.

Exact, bit for bit: n, flags, aabb_min, aabb_max, reserved against the checker; obb_half and obb_center against
obb_from() on the device's own returned centroid and axes.  Within bounds derived from float32 output rounding
(boxes_reference.check_properties states them): centroid, eigenvalues, orthonormality, handedness, the sign rule, the
eigen residual, containment.  Axes are never compared elementwise: equal eigenvalues leave them free."""
import ctypes as C

import numpy as np
import pytest

import boxes_reference as BR
import cluster_reference as CR
import knn_reference as KR

pytestmark = pytest.mark.gpu

NAMES = KR.NAMES + sorted(CR.OWN)


def _host(wm, out):
    """a cluster_boxes result -> structured numpy array"""
    if isinstance(out, np.ndarray):
        return out
    return out.cpu().numpy().reshape(-1).view(wm.BOX_DTYPE)


def _check(wm, ctx, cloud, off, idx=None, clusters=None):
    off = np.asarray(off, np.uint32)
    box = _host(wm, ctx.cluster_boxes(cloud, off, idx))
    ref = BR.boxes(cloud, off, idx)
    BR.check_exact(ref, box, cloud, off, idx, clusters)
    BR.check_properties(ref, box, cloud, off, idx, clusters)
    return box, ref


def _raw(wm, ctx, cloud, off, idx, mem, list_mem, out_mem, n=None, n_members=None):
    """The C entry point itself: cloud (n, k) float32 of any k >= 3 (the stride is 4 k), each array in the memory
    asked for -> (rc, boxes as a structured array)."""
    import torch
    keep = []

    def place(a, where):
        if a is None:
            return None
        a = np.array(a)  # (a writable copy: torch takes no read-only array)
        if where == wm.WM_MEM_HOST:
            keep.append(a)
            return C.c_void_p(a.ctypes.data)
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        keep.append(t)
        return C.c_void_p(t.data_ptr())

    cloud = np.ascontiguousarray(cloud, np.float32)
    off = np.ascontiguousarray(off, np.uint32)
    idx = None if idx is None else np.ascontiguousarray(idx, np.int32)
    nc = len(off) - 1
    n = len(cloud) if n is None else n
    if n_members is None:
        n_members = len(idx) if idx is not None else n
    p_cloud, p_idx, p_off = place(cloud, mem), place(idx, list_mem), place(off, list_mem)
    if out_mem == wm.WM_MEM_DEVICE:
        out = torch.zeros((max(nc, 1), 128), dtype=torch.uint8, device="cuda")
        p_out = C.c_void_p(out.data_ptr())
    else:
        out = np.zeros(max(nc, 1), wm.BOX_DTYPE)
        p_out = C.c_void_p(out.ctypes.data)
    torch.cuda.synchronize()
    rc = wm.lib().wm_cluster_boxes(ctx._h, p_cloud, n, cloud.shape[1] * 4, mem, p_idx, n_members, p_off, nc, list_mem,
                                   p_out, out_mem, None)
    return rc, _host(wm, out)[:nc]


# ------------------------------------------------------------------ 1. the shapes: their clusters, and each as one cluster
@pytest.mark.parametrize("name", NAMES)
def test_shape_clusters_and_whole_cloud(wm, ctx, name):
    cloud = CR.shapes()[name]
    for tol in [t for n, t in CR.CASES if n == name]:
        ref = CR.brute_case(name, tol)
        _check(wm, ctx, cloud, ref["offsets"], ref["indices"])
    box, ref = _check(wm, ctx, cloud, [0, len(cloud)])
    if name == "holes":
        assert box["n"][0] == 2996 and box["flags"][0] == wm.WM_BOX_NONFINITE
    if name == "point":
        assert not box["eigenvalues"].view(np.uint32).any() and np.array_equal(box["axes"][0], np.eye(3, dtype=np.float32))
    if name in ("line", "exact_plane"):
        assert box["eigenvalues"][0][2] <= 2.0 ** -22 * box["eigenvalues"][0][0]


# ------------------------------------------------------------------ 2. every point a cluster of its own
@pytest.mark.parametrize("name", ["scene", "holes", "utm"])
def test_every_point_a_cluster(wm, ctx, name):
    cloud = CR.shapes()[name]
    box, ref = _check(wm, ctx, cloud, np.arange(len(cloud) + 1))
    fin = np.isfinite(cloud).all(1)
    assert np.array_equal(box["n"], fin.astype(np.uint32))
    assert np.array_equal(box["centroid"][fin].view(np.uint32), (cloud[fin] + np.float32(0)).view(np.uint32))
    assert np.array_equal(box["obb_center"][fin].view(np.uint32), (cloud[fin] + np.float32(0)).view(np.uint32))
    assert not box["obb_half"].any() and not box["eigenvalues"].any()


# ------------------------------------------------------------------ 3. runs across wave, chunk and tile edges
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 1023, 1024, 0, 0, 3, 2049, 1]


@pytest.mark.parametrize("shift", [0, 1, 63])
def test_sizes_back_to_back(wm, ctx, shift):
    sizes = ([shift] if shift else []) + SIZES
    off = np.r_[0, np.cumsum(sizes)]
    rng = np.random.default_rng(300 + shift)
    cloud = (rng.normal(0, 1, (off[-1], 3)) * [5, 2, 0.5] + rng.uniform(-50, 50, (1, 3))).astype(np.float32)
    idx = rng.permutation(off[-1]).astype(np.int32)
    box, ref = _check(wm, ctx, cloud, off, idx)
    assert box["n"].tolist() == sizes
    box2, _ = _check(wm, ctx, cloud, off)  # the records in place
    assert box2["n"].tolist() == sizes


# ------------------------------------------------------------------ 4. the large scene: 162 250 clusters, and one of 264 439
@pytest.mark.parametrize("tol", CR.BIG_TOLERANCES)
def test_large_scene(wm, ctx, tol):
    cloud, ref = CR.big_cloud(), CR.big_case(tol)
    size = np.diff(ref["offsets"].astype(np.int64))
    some = sorted(set(np.argsort(-size, kind="stable")[:48].tolist() + list(range(0, len(size), max(len(size) // 400, 1)))))
    box, r = _check(wm, ctx, cloud, ref["offsets"], ref["indices"], clusters=some)
    assert box["n"][0] == ref["largest"] and int(box["n"].sum()) == ref["n_clustered"]
    again = _host(wm, ctx.cluster_boxes(cloud, ref["offsets"], ref["indices"]))
    assert again.tobytes() == box.tobytes()


# ------------------------------------------------------------------ 5. determinism: order inside the clusters, repeats
def test_member_order_and_repeats_change_no_byte(wm, ctx):
    rng = np.random.default_rng(11)
    for name, tol in (("scene", 2.0), ("noisy_plane", 0.5), ("utm", 2.0), ("lattice", 0.5000001)):
        cloud, ref = CR.shapes()[name], CR.brute_case(name, tol)
        off, idx = ref["offsets"], ref["indices"]
        a = _host(wm, ctx.cluster_boxes(cloud, off, idx))
        b = _host(wm, ctx.cluster_boxes(cloud, off, idx))
        assert a.tobytes() == b.tobytes()
        for _ in range(2):
            perm = idx.copy()
            for c in range(len(off) - 1):
                perm[off[c]:off[c + 1]] = rng.permutation(idx[off[c]:off[c + 1]])
            assert _host(wm, ctx.cluster_boxes(cloud, off, perm)).tobytes() == a.tobytes(), name
    cloud, ref = CR.big_cloud(), CR.big_case(0.3)  # one cluster over 259 tiles: the atomics' order is free
    off, idx = ref["offsets"], ref["indices"]
    a = _host(wm, ctx.cluster_boxes(cloud, off, idx))
    perm = idx.copy()
    perm[:off[1]] = rng.permutation(idx[:off[1]])
    assert _host(wm, ctx.cluster_boxes(cloud, off, perm)).tobytes() == a.tobytes()


# ------------------------------------------------------------------ 6. memories, strides, indices or gathered points
def test_memories_strides_and_gathered_points(wm, ctx):
    cloud3, ref = CR.shapes()["holes"], CR.brute_case("holes", 2.0)
    off, idx = ref["offsets"], ref["indices"]
    H, D = wm.WM_MEM_HOST, wm.WM_MEM_DEVICE
    want = None
    for k in (3, 4, 8):
        cloud = np.full((len(cloud3), k), 7.0, np.float32)
        cloud[:, :3] = cloud3
        for mem in (H, D):
            for list_mem in (H, D):
                for out_mem in (H, D):
                    rc, box = _raw(wm, ctx, cloud, off, idx, mem, list_mem, out_mem)
                    assert rc == wm.WM_OK
                    if want is None:
                        want = box.tobytes()
                        r = BR.boxes(cloud3, off, idx)
                        BR.check_exact(r, box, cloud3, off, idx)
                        BR.check_properties(r, box, cloud3, off, idx)
                    assert box.tobytes() == want, (k, mem, list_mem, out_mem)
                    gathered = np.ascontiguousarray(cloud[idx])
                    rc, box = _raw(wm, ctx, gathered, off, None, mem, list_mem, out_mem)
                    assert rc == wm.WM_OK and box.tobytes() == want, (k, mem, list_mem, out_mem, "gathered")
    # the Python surface: torch tensors in, a tensor of bytes out
    import torch
    t_cloud = torch.from_numpy(cloud3.copy()).cuda()
    t_off, t_idx = torch.from_numpy(off.view(np.int32)).cuda(), torch.from_numpy(idx).cuda()
    out = ctx.cluster_boxes(t_cloud, t_off, t_idx)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (len(off) - 1, 128)
    assert _host(wm, out).tobytes() == want
    timing = {}
    assert ctx.cluster_boxes(t_cloud, t_off, t_idx, out_mem=H, timing=timing).tobytes() == want and timing["kernel_ms"] > 0
    assert len(ctx.cluster_boxes(cloud3, np.zeros(1, np.uint32))) == 0


# ------------------------------------------------------------------ 7. lists that are no partition: found on the device
def test_bad_lists_are_argument_errors_and_no_fault(wm, ctx):
    cloud, ref = CR.shapes()["scene"], CR.brute_case("scene", 2.0)
    off, idx = ref["offsets"], ref["indices"]
    good = _host(wm, ctx.cluster_boxes(cloud, off, idx)).tobytes()
    H, D = wm.WM_MEM_HOST, wm.WM_MEM_DEVICE
    descending = off.copy()
    descending[3], descending[4] = off[4], off[3]
    wrong_last = off.copy()
    wrong_last[-1] -= 1
    far = off.copy()
    far[1:-1] = 0xFFFFFF00  # beyond every member, and not ascending into the last
    first = off.copy()
    first[0] = 1
    at_n, negative = idx.copy(), idx.copy()
    at_n[len(idx) // 2] = len(cloud)
    negative[7] = -1
    for mem in (H, D):
        for o, i in ((descending, idx), (wrong_last, idx), (far, idx), (first, idx), (off, at_n), (off, negative)):
            rc, _ = _raw(wm, ctx, cloud, o, i, mem, mem, mem)
            assert rc == wm.WM_ERR_ARG
        rc, _ = _raw(wm, ctx, cloud, off, idx, mem, mem, mem, n=len(cloud) - 1)  # the largest index is now n
        assert rc == wm.WM_ERR_ARG
        rc, box = _raw(wm, ctx, cloud, off, idx, mem, mem, mem)
        assert rc == wm.WM_OK and box.tobytes() == good
    with pytest.raises(wm.WmError):
        ctx.cluster_boxes(cloud, wrong_last, idx)


# ------------------------------------------------------------------ 8. a span the fixed point cannot hold
def test_range_flag_keeps_the_aabb(wm, ctx):
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-10, 10, (400, 3)).astype(np.float32)
    cloud[150] = [2.0 ** 21 - 10, 0, 0]        # cluster 1 spans 2^21 m and a little
    cloud[160] = [-10.0, 0, 0]
    cloud[350, 1] = np.float32(2.0 ** 20) - 10  # cluster 3 stays just inside: its span is below 2^20
    cloud[351, 1] = -9.5
    off = [0, 100, 200, 300, 400]
    box, ref = _check(wm, ctx, cloud, off)
    assert box["flags"].tolist() == [0, wm.WM_BOX_RANGE, 0, 0] and box["n"].tolist() == [100] * 4
    assert box["aabb_max"][1][0] == np.float32(2.0 ** 21 - 10) and box["aabb_min"][1][0] == -10.0
    assert not box["axes"][1].any() and box["eigenvalues"][3][0] > 1e9
    exact = np.float32([[0, 0, 0], [2.0 ** 20, 0, 0]])  # a span of exactly 2^20 is out of range
    assert _host(wm, ctx.cluster_boxes(exact, np.array([0, 2], np.uint32)))["flags"][0] == wm.WM_BOX_RANGE


# ------------------------------------------------------------------ 9. the context
def test_state_is_not_touched(wm):
    from libwave_amd import synth
    ref_cloud, tgt_cloud, _ = synth.pair(6000, seed=21, mode="resample")
    third = CR.shapes()["clumps_outliers"]
    runs = []
    for with_boxes in (True, False):
        c = wm.Context(0)
        try:
            c.set_source(ref_cloud)
            c.set_target(tgt_cloud)
            a = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            corr1 = c.correspondences()
            o1 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            k1 = c.cluster_extract(third, tolerance=0.5)
            n1 = c.estimate_normals(1)
            if with_boxes:
                b1 = c.cluster_boxes(third, k1["offsets"], k1["indices"])
                b2 = c.cluster_boxes(tgt_cloud, np.array([0, len(tgt_cloud)], np.uint32))
                assert len(b1) == 14 and b2["n"][0] == len(tgt_cloud)
            n2 = c.estimate_normals(1)
            corr2 = c.correspondences()
            o2 = c.outlier_filter(third, method=1, radius=0.5, min_neighbors=5)
            k2 = c.cluster_extract(third, tolerance=0.5)
            b = c.icp_align(max_corr=3.0, mode=wm.WM_ICP_PLANE)
            assert n1.tobytes() == n2.tobytes() and c.sizes() == (len(ref_cloud), len(tgt_cloud))
            for x, y in zip(corr1, corr2):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
            for k in ("indices", "labels", "counts"):
                assert o1[k].tobytes() == o2[k].tobytes()
            for k in ("indices", "labels", "offsets"):
                assert k1[k].tobytes() == k2[k].tobytes()
            runs.append((a, b, o2, n2, k2))
        finally:
            c.close()
    (a1, b1, o1, n1, k1), (a2, b2, o2, n2, k2) = runs
    for x, y in ((a1, a2), (b1, b2)):
        assert x["rc"] == y["rc"] == wm.WM_OK
        assert x["T"].tobytes() == y["T"].tobytes() and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"]
    assert o1["indices"].tobytes() == o2["indices"].tobytes() and n1.tobytes() == n2.tobytes()
    assert k1["indices"].tobytes() == k2["indices"].tobytes()


# ------------------------------------------------------------------ 10. the pipeline in device memory
def test_ground_batch_into_cluster_batch_into_boxes(wm, ctx):
    import torch
    import ground_scenes as S
    scans = [torch.from_numpy(S.rings_sensor_frame(20_000, seed=42 + k)).cuda() for k in range(4)]
    _, kept, goff = ctx.ground_segment_batch(scans, points=True)
    slices = [kept[goff[k]:goff[k + 1]] for k in range(4)]
    got, pts, poff = ctx.cluster_extract_batch(slices, points=True, tolerance=0.5, min_cluster_size=20)
    assert pts.is_cuda
    # the batch-wide offsets, in device memory: each scan's own, moved to where its members start
    d_off = torch.cat([got[k]["offsets"][(1 if k else 0):] + int(poff[k]) for k in range(4)])
    n_clusters = sum(g["n_clusters"] for g in got)
    assert d_off.is_cuda and len(d_off) == n_clusters + 1 and n_clusters > 8
    on_device = ctx.cluster_boxes(pts, d_off)  # one call for the clusters of all scans
    assert on_device.is_cuda
    dev = _host(wm, on_device)
    # the same through the host, scan by scan, from the indices and the scans' own points
    rows = []
    for k in range(4):
        host = slices[k].cpu().numpy()
        rows.append(ctx.cluster_boxes(host, got[k]["offsets"].cpu().numpy().view(np.uint32), got[k]["indices"].cpu().numpy()))
    through_host = np.concatenate(rows)
    assert through_host.tobytes() == dev.tobytes()
    h_pts, h_off = pts.cpu().numpy(), d_off.cpu().numpy().view(np.uint32)
    r = BR.boxes(h_pts, h_off)
    BR.check_exact(r, dev, h_pts, h_off)
    BR.check_properties(r, dev, h_pts, h_off)
