"""pcl::VoxelGrid on the device (voxel_downsample_dev, libwave_amd/csrc/wm_voxel.hip; the batched k_vb_*, wm_batch.hip) and
its neighbours wm_transform_cloud / k_unpack held to tests/voxel_reference.py on the shapes where such kernels go wrong:
every leaf size around the centroid kernels' trips (8 points a lane, 64 a wave), the hand-over between the two kernels
at n_valid = 24 leaves and one point past it, more leaves than waves launched, more points than the own radix sort's
threshold, one leaf, points on leaf boundaries and one float beside them, leaf indices beyond 2^24, lattices of 2^31 ..
2^32 cells and of 2^32 and more (PCL's `unsigned int` index: arithmetic mod 2^32), non-finite rows, every record layout.

Every comparison is of bytes: the same shape, the same float32 bits as the reference, no tolerance.  One exception that is
the library's stated behaviour, not slack: where PCL's size rule fires and the cloud comes back unfiltered, the device's
copy of a NON-FINITE row is all-NaN (k_pack turns such rows into NaN on the way in); the finite rows are held to their
bytes, in place and in order, the non-finite ones to being non-finite.  The same holds for wm_transform_cloud's rows.

tests/test_voxel_reference_cpu.py holds the reference to the C oracle on the same clouds."""
import ctypes as C
import time

import numpy as np
import pytest
import torch  # (before the HIP library is loaded: see test_fullsize_gpu.py)

import voxel_reference as VR
from helpers import pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu

RADIX_MIN_DEFAULT = 256 << 10
SENTINEL = np.uint32(0xA5A5A5A5)
EMPTY = np.zeros((0, 3), np.float32)


def _three_ways(ctx, cloud, leaf):
    """the filter with the library's own radix sort, with rocPRIM's, and with the default choice between them"""
    out = []
    try:
        for radix_min in (0, 1 << 30, None):
            ctx.set_option("radix_min", RADIX_MIN_DEFAULT if radix_min is None else radix_min)
            out.append(ctx.voxel_downsample(cloud, leaf))
    finally:
        ctx.set_option("radix_min", RADIX_MIN_DEFAULT)
    return out


def _first_difference(got, want):
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    return "ok" if len(bad) == 0 else "%d of %d rows differ, first %d: %s, expected %s" % (len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


FILTERED = [n for n in VR.SMALL if n != "cube_past_the_rule"]


@pytest.mark.parametrize("name", FILTERED)
def test_every_small_shape_with_either_sort(ctx, name):
    cloud, leaf, want = VR.shape(name)
    own, rocprim, default = _three_ways(ctx, cloud, leaf)
    assert VR.same_bytes(own, want), (name, "own sort", _first_difference(own, want))
    assert VR.same_bytes(rocprim, want), (name, "rocPRIM", _first_difference(rocprim, want))
    assert VR.same_bytes(default, want), (name, "default", _first_difference(default, want))


def test_more_leaves_than_waves_and_more_points_than_radix_min(ctx):
    """10 500 leaves of 25 points: the wave kernel's grid-stride loop wraps (8 192 waves), the own sort runs unasked"""
    cloud, leaf, want = VR.shape("many_leaves")
    ctx.voxel_downsample(cloud[:1000], leaf)  # (the library's first call on a context sets its buffers up)
    t0 = time.perf_counter()
    got = ctx.voxel_downsample(cloud, leaf)
    dt = time.perf_counter() - t0
    print("262 500 points, 10 500 leaves: %.3f s" % dt)
    assert VR.same_bytes(got, want), _first_difference(got, want)
    assert dt < 5.0, dt


def test_unfiltered_branch_keeps_finite_rows_and_non_finite_rows_stay_non_finite(ctx):
    cloud, leaf, want = VR.shape("cube_past_the_rule")
    assert VR.same_bytes(want, cloud)
    fin = np.isfinite(cloud).all(1)
    assert 0 < fin.sum() < len(cloud)
    for got in _three_ways(ctx, cloud, leaf):
        assert got.shape == cloud.shape
        assert VR.same_bytes(got[fin], cloud[fin])  # in place, in order
        assert not np.isfinite(got[~fin]).all(1).any()  # (all-NaN on the device: see the header)


# ------------------------------------------------------------------------------------------------------ entry points
def _reference(cloud, leaf):
    return VR.voxel_grid(cloud, leaf) if len(cloud) else EMPTY


@pytest.mark.parametrize("leaf", [0.8, 1.0, 0.25, 0.1, 0.05])
def test_shapes_as_items_of_one_batched_call(ctx, leaf):
    """several clouds per call, an empty one among them, small lattices beside the 1291^3 one (one sort key carries the
    cloud number above the widest leaf index of the batch)"""
    names = [n for n in VR.SMALL if VR.LEAF_SIZES[n][1] == leaf and
             n.split("_")[0] in ("ladder", "threshold", "boundaries", "far", "cube") and n != "cube_past_the_rule"]
    assert names, leaf
    clouds = [VR.shape(n)[0] for n in names] + [VR.shape("ladder_lane")[0], EMPTY, VR.shape("holes_y")[0]]
    if len(clouds) % 2:
        clouds.append(VR.shape("threshold_past")[0])
    pairs = [(clouds[k], clouds[k + 1]) for k in range(0, len(clouds), 2)]
    got = ctx.voxel_downsample_batch(pairs, leaf)
    flat = [c for pair in got for c in pair]
    assert len(flat) == len(clouds)
    for k, (cloud, g) in enumerate(zip(clouds, flat)):
        want = _reference(cloud, leaf)
        assert VR.same_bytes(g, want), (leaf, k, _first_difference(g, want))


@pytest.mark.parametrize("name", VR.WIDE)
def test_a_lattice_of_2_to_the_32_cells_is_refused_by_the_batched_filter(wm, ctx, name):
    cloud, leaf, want = VR.shape(name)
    small = VR.shape("ladder_lane")[0]
    items = (wm.BatchItem * 2)()
    items[0].src, items[0].n_src, items[0].target, items[0].n_target = small.ctypes.data, len(small), cloud.ctypes.data, len(cloud)
    items[1].src, items[1].n_src, items[1].target, items[1].n_target = small.ctypes.data, len(small), small.ctypes.data, len(small)
    cap = 2 * len(cloud) + 6 * len(small)
    out = np.empty((cap, 3), np.float32)
    counts = (C.c_size_t * 4)()
    rc = wm.lib().wm_voxel_downsample_batch(ctx._h, items, 2, 12, wm.WM_MEM_HOST, C.c_float(leaf),
                                            out.ctypes.data_as(C.POINTER(C.c_float)), cap, counts)
    assert rc == wm.WM_ERR_ARG


@pytest.mark.parametrize("name", VR.WIDE)
def test_batched_match_hands_such_a_pair_to_the_one_pair_path(wm, ctx, name):
    cloud, leaf, want = VR.shape(name)
    target = (cloud + np.float32([0.05, -0.03, 0.0])).astype(np.float32)
    a, b, _ = synth.pair(3000, seed=9, mode="resample")
    pairs = [(a, b), (cloud, target), (b, a)]
    kw = dict(res=leaf, multiscale_steps=0, max_corr=3.0, max_iter=30)
    got = ctx.icp_batch_match(pairs, with_info=False, **kw)
    for k, ((ref, tgt), g) in enumerate(zip(pairs, got)):
        fresh = wm.Context(0)
        one = fresh.icp_match(ref, tgt, carry_state=1, **kw)
        sizes = fresh.sizes()
        fresh.close()
        assert g["rc"] == one["rc"], (name, k, g["rc"], one["rc"])
        assert (g["iterations"], g["state"], g["n_corr"]) == (one["iterations"], one["state"], one["n_corr"]), (name, k)
        if k == 1:  # the same code on the same clouds: status and transform to the bit
            assert (g["T"] is None) == (one["T"] is None) and (one["T"] is None or np.array_equal(g["T"], one["T"])), name
        elif one["rc"] == 0:  # its neighbours stay in the resident kernel (sums in another order: test_batch_gpu.py's bound)
            dt, ang = pose_error(g["T"], one["T"])
            assert dt <= 1e-6 and ang <= 1e-7, (name, k, dt, ang)
        if k == 1:  # match()'s own filter: the clouds it registered are the reference's leaves
            assert sizes == (len(want), len(VR.voxel_grid(target, leaf))), (name, sizes)


@pytest.mark.parametrize("name", ["ladder_wave", "ladder_lane", "flat"])
def test_filtered_setters_keep_the_reference_number_of_leaves(wm, ctx, name):
    cloud, leaf, want = VR.shape(name)
    other = VR.shape("holes_z")[0]
    L = wm.lib()
    assert L.wm_set_source_filtered(ctx._h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, wm.WM_MEM_HOST, C.c_float(leaf)) == 0
    assert L.wm_set_target_filtered(ctx._h, C.c_void_p(other.ctypes.data), len(other), 12, wm.WM_MEM_HOST, C.c_float(leaf)) == 0
    assert ctx.sizes() == (len(want), len(VR.voxel_grid(other, leaf)))
    assert L.wm_set_target_filtered(ctx._h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, wm.WM_MEM_HOST, C.c_float(leaf)) == 0
    assert L.wm_set_source_filtered(ctx._h, C.c_void_p(other.ctypes.data), len(other), 12, wm.WM_MEM_HOST, C.c_float(leaf)) == 0
    assert ctx.sizes() == (len(VR.voxel_grid(other, leaf)), len(want))


# ----------------------------------------------------------------------------------------------------------- layouts
def _records(cloud, stride):
    """the cloud as records of `stride` bytes; what lies beyond xyz is NaN: nothing may read it"""
    rec = np.full((len(cloud), stride // 4), np.nan, np.float32)
    rec[:, :3] = cloud
    return rec


class _Buffer:
    """input records / a sentinel-filled destination in host or device memory"""

    def __init__(self, host, mem_device):
        self.host = np.ascontiguousarray(host)
        self.dev = torch.from_numpy(self.host.view(np.float32)).cuda() if mem_device else None
        if mem_device:
            torch.cuda.synchronize()  # (the context's stream is not torch's)

    @property
    def ptr(self):
        return self.dev.data_ptr() if self.dev is not None else self.host.ctypes.data

    def fetch(self):
        return self.dev.cpu().numpy().view(np.uint32) if self.dev is not None else self.host.view(np.uint32)


def _check_records(raw, want, out_stride, device_dest, tag):
    """raw: the destination's words [cap, out_stride / 4] after the call; want [m, 3] float32"""
    m, words = len(want), out_stride // 4
    assert VR.same_bytes(raw[:m, :3], want.view(np.uint32)), (tag, _first_difference(raw[:m, :3].view(np.float32), want))
    if words >= 4:
        assert (raw[:m, 3].view(np.float32) == 1.0).all(), tag  # pcl::PointXYZ's data[3]
    if words > 4:  # a host destination is zero beyond byte 16, a device destination is left as the caller filled it
        assert (raw[:m, 4:] == (SENTINEL if device_dest else 0)).all(), tag
    assert (raw[m:] == SENTINEL).all(), tag  # nothing beyond the last record


@pytest.mark.parametrize("mem,out_mem", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_voxel_downsample_in_every_layout(wm, ctx, mem, out_mem):
    cloud, leaf, want = VR.shape("ladder_lane")
    cap = len(want) + 3
    for stride in (12, 16, 32):
        src = _Buffer(_records(cloud, stride), mem == wm.WM_MEM_DEVICE)
        for out_stride in (12, 16, 32):
            dst = _Buffer(np.full((cap, out_stride // 4), SENTINEL, np.uint32), out_mem == wm.WM_MEM_DEVICE)
            m = C.c_size_t(0)
            rc = wm.lib().wm_voxel_downsample(ctx._h, C.c_void_p(src.ptr), len(cloud), stride, mem, C.c_float(leaf),
                                              C.c_void_p(dst.ptr), out_stride, out_mem, cap, C.byref(m))
            assert rc == 0 and m.value == len(want), (stride, out_stride, rc, m.value)
            _check_records(dst.fetch(), want, out_stride, out_mem == wm.WM_MEM_DEVICE, (stride, out_stride))


def test_voxel_downsample_refuses_a_destination_that_is_too_small(wm, ctx):
    cloud, leaf, want = VR.shape("ladder_lane")
    out = np.full((len(want), 3), SENTINEL, np.uint32)
    m = C.c_size_t(0)
    rc = wm.lib().wm_voxel_downsample(ctx._h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, wm.WM_MEM_HOST, C.c_float(leaf),
                                      C.c_void_p(out.ctypes.data), 12, wm.WM_MEM_HOST, len(want) - 1, C.byref(m))
    assert rc == wm.WM_ERR_ARG and (out == SENTINEL).all()
    rc = wm.lib().wm_voxel_downsample(ctx._h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, wm.WM_MEM_HOST, C.c_float(leaf),
                                      C.c_void_p(out.ctypes.data), 12, wm.WM_MEM_HOST, len(want), C.byref(m))
    assert rc == 0 and m.value == len(want) and VR.same_bytes(out.view(np.float32), want)


T_GENERAL = synth.make_T((0.2, -3.0, 1.5), (0.3, -0.2, 1.1))  # no zero among the rotation's entries


@pytest.mark.parametrize("mem,out_mem", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_transform_cloud_in_every_layout(wm, ctx, oracle, mem, out_mem):
    cloud = VR.shape("ladder_lane")[0]
    want = oracle.transform_cloud_d(cloud, T_GENERAL)
    T = np.ascontiguousarray(T_GENERAL, np.float64)
    cap = len(cloud) + 3
    for stride in (12, 16, 32):
        src = _Buffer(_records(cloud, stride), mem == wm.WM_MEM_DEVICE)
        for out_stride in (12, 16, 32):
            dst = _Buffer(np.full((cap, out_stride // 4), SENTINEL, np.uint32), out_mem == wm.WM_MEM_DEVICE)
            rc = wm.lib().wm_transform_cloud(ctx._h, C.c_void_p(src.ptr), len(cloud), stride, mem,
                                             T.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(dst.ptr), out_stride, out_mem)
            assert rc == 0, (stride, out_stride, rc)
            _check_records(dst.fetch(), want, out_stride, out_mem == wm.WM_MEM_DEVICE, (stride, out_stride))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_transform_cloud_around_one_workgroup_with_non_finite_rows(ctx, oracle, n):
    """finite rows: the oracle's bytes.  A row with a NaN is all-NaN on both sides.  A row with an infinity is non-finite
    in every coordinate on both sides (the rotation has no zero entry): infinities or NaN in the oracle, NaN on the
    device, whose k_pack has made the row NaN before the transform sees it."""
    rng = np.random.default_rng(n)
    cloud = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    bad = {0: [np.nan, 1, 2], n // 2: [3, np.inf, 4], n - 1: [5, 6, -np.inf]} if n > 1 else {0: [1, np.nan, 2]}
    for row, v in bad.items():
        cloud[row] = v
    got, want = ctx.transform_cloud(cloud, T_GENERAL), oracle.transform_cloud_d(cloud, T_GENERAL)
    fin = np.isfinite(cloud).all(1)
    assert fin.sum() == n - len(bad)
    assert VR.same_bytes(got[fin], want[fin])
    assert not np.isfinite(want[~fin]).any() and not np.isfinite(got[~fin]).any()
    nan_rows = np.isnan(cloud).any(1)
    assert np.isnan(got[nan_rows]).all() and np.isnan(want[nan_rows]).all()
    # and on finite clouds of these sizes, every byte
    clean = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    assert VR.same_bytes(ctx.transform_cloud(clean, T_GENERAL), oracle.transform_cloud_d(clean, T_GENERAL))
