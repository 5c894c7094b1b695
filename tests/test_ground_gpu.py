"""wm_ground_segment (libwave_amd/csrc/wm_ground.hip) against the float64 checker tests/ground_reference.py:
labels, the ordered indices of every keep mask and every stat must be EQUAL, on the reference's fixture, the ring
scans, a large-model case and the edge cases.  Each case first asserts that the checker's decisions and bins are
far from their thresholds (margins above 1e-9): there a Cholesky solve and an LU solve, and the device's atan2
and numpy's, cannot disagree -- so anything but equality is a bug."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_reference as G  # noqa: E402
import ground_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

MASKS = range(8)
STAT_KEYS = ("n_ground", "n_obstacle", "n_overhanging", "n_in_range", "n_signal_cells", "n_model_cells",
             "n_sufficient_sectors", "passes_total", "passes_max")


@pytest.fixture(scope="module")
def fixture_cloud(testscan):
    return G.car_box_removal(testscan)


def check(ctx, pts, params=None, masks=MASKS, device_input=False):
    P = dict(G.default_params(), **(params or {}))
    ref = G.segment(np.asarray(pts)[:, :3] if len(pts) else np.zeros((0, 3), np.float32), P)
    assert ref["margin"] > 1e-9 and ref["bin_margin"] > 1e-9, (ref["margin"], ref["bin_margin"])
    cloud = pts
    if device_input:
        import torch
        cloud = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda")
    for keep in masks:
        labels, idx, st = ctx.ground_segment(cloud, P, keep=keep)
        np.testing.assert_array_equal(labels, ref["labels"])
        want = [ref[name] for bit, name in ((1, "ground"), (2, "obstacle"), (4, "overhanging")) if keep & bit]
        want = np.concatenate(want) if want else np.zeros(0, np.int32)
        np.testing.assert_array_equal(idx, want, err_msg="keep mask %d" % keep)
        for k in STAT_KEYS:
            assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])
    return ref


def test_fixture_with_the_test_yaml(ctx, fixture_cloud):
    ref = check(ctx, fixture_cloud, G.load_yaml(S.YAML))
    assert ref["stats"]["passes_max"] >= 2 and ref["stats"]["n_ground"] > 10000


def test_fixture_with_the_defaults(ctx, fixture_cloud):
    check(ctx, fixture_cloud)


def test_fixture_as_xyzw_records(ctx, fixture_cloud):  # stride 16
    pts4 = np.concatenate([fixture_cloud, np.ones((len(fixture_cloud), 1), np.float32)], axis=1)
    check(ctx, pts4, G.load_yaml(S.YAML), masks=(G.KEEP_DEFAULT,))


def test_fixture_from_device_memory(ctx, fixture_cloud):
    check(ctx, fixture_cloud, G.load_yaml(S.YAML), masks=(G.KEEP_DEFAULT, 7), device_input=True)


def test_rings_130k(ctx):
    check(ctx, S.rings_sensor_frame(130_000), masks=(G.KEEP_DEFAULT, 7, 1))


def test_rings_1m(ctx):
    check(ctx, S.rings_sensor_frame(1_000_000), masks=(G.KEEP_DEFAULT, 7))


def test_large_model(ctx):
    ref = check(ctx, S.large_model(), dict(num_bins_a=8, num_bins_l=400), masks=(G.KEEP_DEFAULT, 7))
    assert ref["stats"]["n_model_cells"] > 8 * 200  # final models of ~400 cells (one pass from the 10 seeds)


def test_large_factor(ctx):
    # every eligible cell a seed: each sector's one pass solves with a factor of ~240 rows (231 KB packed, beyond
    # the 160 KiB of LDS; the >256-row loops of the sector kernel)
    P = dict(num_bins_a=8, num_bins_l=400, num_seed_points=-1, max_seed_range=60.0)
    ref = check(ctx, S.large_model(), P, masks=(G.KEEP_DEFAULT, 7))
    assert ref["factor_rows"] > 200


def test_large_factor_extended(ctx):
    # a tight p_tdata: the model grows a few cells per pass (18 passes), each extending a factor of more than 256 rows
    P = dict(num_bins_a=4, num_bins_l=600, num_seed_points=-1, max_seed_range=60.0, p_tdata=1.0)
    ref = check(ctx, S.large_model(), P, masks=(G.KEEP_DEFAULT, 7))
    assert ref["extended_from"] > 256 and ref["stats"]["passes_max"] > 5


def test_empty_and_all_nan(ctx):
    labels, idx, st = ctx.ground_segment(np.zeros((0, 3), np.float32))
    assert len(labels) == 0 and len(idx) == 0 and st["n_in_range"] == 0
    nan = np.full((1000, 3), np.nan, np.float32)
    labels, idx, st = ctx.ground_segment(nan, keep=7)
    assert (labels == 0).all() and len(idx) == 0 and all(st[k] == 0 for k in STAT_KEYS)


def test_rmax_5m(ctx, fixture_cloud):
    ref = check(ctx, fixture_cloud, dict(G.load_yaml(S.YAML), rmax=5.0), masks=(G.KEEP_DEFAULT, 7))
    assert 0 < ref["stats"]["n_in_range"] < len(fixture_cloud)


@pytest.mark.parametrize("name", ["disc", "structures", "counts", "seeds0", "seeds1", "seeds_all", "tie",
                                  "signed_zero", "sectors7", "single_seed"])
def test_small_scenes(ctx, name):
    import test_ground_reference_cpu as T
    pts, params = T.SCENES[name]()
    check(ctx, pts, params)


def test_signed_zero_second_order(ctx):
    # -0.0 before +0.0: the first zero is still the prototype (the seed-range test in the scene tells which one won)
    import test_ground_reference_cpu as T
    pts, params = T.scene_signed_zero(neg_first=True)
    ref = check(ctx, pts, params)
    assert ref["stats"]["n_sufficient_sectors"] == 1


def test_two_calls_identical(ctx, fixture_cloud):
    a = ctx.ground_segment(fixture_cloud, G.load_yaml(S.YAML), keep=7)
    b = ctx.ground_segment(fixture_cloud, G.load_yaml(S.YAML), keep=7)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


@pytest.mark.parametrize("bad", [dict(num_bins_a=0), dict(num_bins_l=-3), dict(p_l=0.0), dict(p_sf=-1.0),
                                 dict(p_sn=0.0), dict(rmax=float("inf")), dict(p_tg=float("nan")),
                                 dict(robot_height=float("nan"))])
def test_bad_parameters(ctx, wm, bad):
    import ctypes as C
    pts = np.zeros((10, 3), np.float32)
    p = wm.ground_params(bad)
    m = C.c_size_t(0)
    out = np.zeros(10, np.int32)
    rc = wm.lib().wm_ground_segment(ctx._h, C.c_void_p(pts.ctypes.data), 10, 12, wm.WM_MEM_HOST, C.byref(p), 6,
                                    C.c_void_p(out.ctypes.data), 10, wm.WM_MEM_HOST, C.byref(m), None, None)
    assert rc == wm.WM_ERR_ARG
    assert not G.params_valid(dict(G.default_params(), **bad))


def test_registration_state_untouched(wm, fixture_cloud):
    """A segmentation between set_target and icp_align, and between two aligns, leaves the registrations
    bit-identical to a context that never segmented."""
    from libwave_amd import synth
    ref, tgt, _ = synth.pair(20000, seed=7, mode="resample")
    kw = dict(max_corr=3.0, force_iterations=12, nn_method=wm.WM_NN_GRID)
    a = wm.Context(0)
    a.set_source(ref)
    a.set_target(tgt)
    want = [a.icp_align(**kw), a.icp_align(**kw)]
    a.close()
    b = wm.Context(0)
    b.set_source(ref)
    b.set_target(tgt)
    b.ground_segment(S.rings_sensor_frame(130_000), keep=7)
    got = [b.icp_align(**kw)]
    b.ground_segment(fixture_cloud, keep=7)
    got.append(b.icp_align(**kw))
    b.close()
    for g, w in zip(got, want):
        assert g["rc"] == w["rc"] == 0
        np.testing.assert_array_equal(g["T"], w["T"])
