"""wm_ground_segment_batch (libwave_amd/csrc/wm_ground.hip): a queue of scans through one sequence of launches.
Every scan's labels, ordered indices and stats must be EQUAL both to wm_ground_segment on that scan alone and to the
float64 checker tests/ground_reference.py -- after the checker's margins are asserted above 1e-9 per scan, as
tests/test_ground_gpu.py::check does: a batch changes neither the arithmetic nor the order inside a scan, so there is
no tolerance anywhere in this file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_reference as G  # noqa: E402
import ground_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_ground", "n_obstacle", "n_overhanging", "n_in_range", "n_signal_cells", "n_model_cells",
             "n_sufficient_sectors", "passes_total", "passes_max")
LARGE = dict(num_bins_a=8, num_bins_l=400, num_seed_points=-1, max_seed_range=60.0)


def drive_scans(fixture, steps=8):
    """The fixture as seen from a moving car: step k = yaw 0.01 k rad about z, then (0.2 k, 0.05 k, 0) m."""
    out = []
    for k in range(steps):
        c, s = np.cos(0.01 * k), np.sin(0.01 * k)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        p = fixture.astype(np.float64) @ R.T + np.array([0.2 * k, 0.05 * k, 0.0])
        out.append(np.ascontiguousarray(p.astype(np.float32)))
    return out


@pytest.fixture(scope="module")
def drive(testscan):
    return drive_scans(G.car_box_removal(testscan))


_REFS = {}


def reference(pts, P, tag):
    """The checker's result for one scan, its margins asserted; kept per (tag) for the tests that share scans."""
    if tag not in _REFS:
        ref = G.segment(np.asarray(pts)[:, :3] if len(pts) else np.zeros((0, 3), np.float32), P)
        assert ref["margin"] > 1e-9 and ref["bin_margin"] > 1e-9, (tag, ref["margin"], ref["bin_margin"])
        _REFS[tag] = ref
    return _REFS[tag]


def want_indices(ref, keep):
    want = [ref[name] for bit, name in ((1, "ground"), (2, "obstacle"), (4, "overhanging")) if keep & bit]
    return np.concatenate(want) if want else np.zeros(0, np.int32)


def to_device(scans):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(s)).to("cuda") for s in scans]


def check_batch(ctx, scans, params, masks, tags, clouds=None):
    """batch == the single call scan by scan == the checker, for every mask."""
    P = dict(G.default_params(), **(params or {}))
    refs = [reference(s, P, t) for s, t in zip(scans, tags)]
    clouds = scans if clouds is None else clouds
    for keep in masks:
        got = ctx.ground_segment_batch(clouds, P, keep=keep)
        assert len(got) == len(scans)
        for k, (labels, idx, st) in enumerate(got):
            ref = refs[k]
            one = ctx.ground_segment(scans[k], P, keep=keep)
            msg = "scan %d, keep mask %d" % (k, keep)
            np.testing.assert_array_equal(labels, one[0], err_msg=msg)
            np.testing.assert_array_equal(idx, one[1], err_msg=msg)
            assert st == one[2], (msg, st, one[2])
            np.testing.assert_array_equal(labels, ref["labels"], err_msg=msg)
            np.testing.assert_array_equal(idx, want_indices(ref, keep), err_msg=msg)
            for key in STAT_KEYS:
                assert st[key] == ref["stats"][key], (msg, key, st[key], ref["stats"][key])
    return refs


def test_drive_of_the_fixture(ctx, drive):
    refs = check_batch(ctx, drive, G.load_yaml(S.YAML), (G.KEEP_DEFAULT, 7, 1), ["drive%d" % k for k in range(8)])
    passes = [r["stats"]["passes_max"] for r in refs]
    assert min(passes) >= 2 and len(set(passes)) > 1, passes  # the scans of one batch run different numbers of passes


@pytest.mark.parametrize("reverse", [False, True])
def test_ragged_sizes_with_the_defaults(ctx, reverse):
    sizes = [(1_000, 7), (20_000, 7), (60_000, 7), (130_000, 42), (250_000, 7)]
    scans = [S.rings_sensor_frame(n, seed) for n, seed in sizes]
    tags = ["rings%d_%d" % ns for ns in sizes]
    scans += [np.zeros((0, 3), np.float32), np.full((1000, 3), np.nan, np.float32)]
    tags += ["empty", "nan"]
    if reverse:
        scans, tags = scans[::-1], tags[::-1]
    check_batch(ctx, scans, None, (G.KEEP_DEFAULT, 7), tags)
    got = ctx.ground_segment_batch(scans, keep=7)
    for k, t in enumerate(tags):
        if t in ("empty", "nan"):
            assert len(got[k][1]) == 0 and (got[k][0] == 0).all() and all(got[k][2][key] == 0 for key in STAT_KEYS)


def test_factor_workspace_across_scans(wm):
    """A fresh context whose first call needs ~45 MB of factors against the 8 MiB the workspace starts with: the
    sector stage runs twice, with blocks of several scans in flight; the second call finds the room it needs."""
    scans = [S.large_model(seed=seed) for seed in (5, 6, 7)]
    P = dict(G.default_params(), **LARGE)
    refs = [reference(s, P, "large%d" % k) for k, s in enumerate(scans)]
    assert all(r["factor_rows"] > 200 for r in refs)
    c = wm.Context(0)
    try:
        first = c.ground_segment_batch(scans, P, keep=7)
        again = c.ground_segment_batch(scans, P, keep=7)
        for k in range(3):
            for got in (first[k], again[k]):
                np.testing.assert_array_equal(got[0], refs[k]["labels"])
                np.testing.assert_array_equal(got[1], want_indices(refs[k], 7))
                for key in STAT_KEYS:
                    assert got[2][key] == refs[k]["stats"][key], (k, key)
            one = c.ground_segment(scans[k], P, keep=7)
            np.testing.assert_array_equal(first[k][0], one[0])
            np.testing.assert_array_equal(first[k][1], one[1])
            assert first[k][2] == one[2]
    finally:
        c.close()


def test_batch_of_one_twice_device_and_stride(ctx, drive):
    P = G.load_yaml(S.YAML)
    tags = ["drive%d" % k for k in range(8)]
    check_batch(ctx, drive[:1], P, (G.KEEP_DEFAULT, 7), tags[:1])
    a = ctx.ground_segment_batch(drive, P, keep=7)
    b = ctx.ground_segment_batch(drive, P, keep=7)
    import torch
    dev = to_device(drive)
    pad = torch.empty(12345, device="cuda")  # (separate allocations, not one block cut into scans)
    d = ctx.ground_segment_batch(dev, P, keep=7)
    del pad
    four = [np.concatenate([s, np.ones((len(s), 1), np.float32)], axis=1) for s in drive]
    e = ctx.ground_segment_batch(four, P, keep=7)
    f = ctx.ground_segment_batch(to_device(four), P, keep=7)
    for other in (b, d, e, f):
        for k in range(8):
            np.testing.assert_array_equal(other[k][0], a[k][0])
            np.testing.assert_array_equal(other[k][1], a[k][1])
            assert other[k][2] == a[k][2]
    check_batch(ctx, drive, P, (7,), tags, clouds=dev)


@pytest.mark.parametrize("width", [3, 4])
def test_points_out(ctx, drive, width):
    P = G.load_yaml(S.YAML)
    scans = drive[:4] + [np.zeros((0, 3), np.float32)] + drive[4:]
    if width == 4:
        scans = [np.concatenate([s, np.full((len(s), 1), 7.0, np.float32)], axis=1) for s in scans]
    plain = ctx.ground_segment_batch(scans, P)
    for clouds in (scans, to_device(scans)):
        res, kept, offs = ctx.ground_segment_batch(clouds, P, points=True)
        kept = kept if isinstance(kept, np.ndarray) else kept.cpu().numpy()
        assert kept.shape == (offs[-1], width) and len(offs) == len(scans) + 1 and offs[0] == 0
        for k, s in enumerate(scans):
            np.testing.assert_array_equal(res[k][0], plain[k][0])
            np.testing.assert_array_equal(res[k][1], plain[k][1])
            assert res[k][2] == plain[k][2] and offs[k + 1] - offs[k] == len(plain[k][1])
            mine = kept[offs[k]:offs[k + 1]]
            np.testing.assert_array_equal(mine[:, :3].view(np.uint32), s[plain[k][1]][:, :3].view(np.uint32))
            if width == 4:  # bytes of a record beyond x y z are zero
                assert (mine[:, 3].view(np.uint32) == 0).all()


def test_the_chain_to_icp_batch_match(ctx, wm, drive):
    """filter on the device -> the kept clouds' slices straight into wm_icp_batch_match(mem = WM_MEM_DEVICE)."""
    P = G.load_yaml(S.YAML)
    res, kept, offs = ctx.ground_segment_batch(to_device(drive), P, points=True)
    dev_clouds = [kept[offs[k]:offs[k + 1]] for k in range(8)]
    host_clouds = [drive[k][res[k][1]] for k in range(8)]
    assert all(0 < len(c) <= wm.WM_BATCH_MAX_TARGET_POINTS for c in host_clouds), [len(c) for c in host_clouds]
    got = ctx.icp_batch_match([(dev_clouds[k + 1], dev_clouds[k]) for k in range(7)], res=-1)
    want = ctx.icp_batch_match([(host_clouds[k + 1], host_clouds[k]) for k in range(7)], res=-1)
    for g, w in zip(got, want):
        assert g["rc"] == w["rc"] and g["iterations"] == w["iterations"] and g["state"] == w["state"]
        assert (g["T"] is None) == (w["T"] is None)
        if w["T"] is not None:
            np.testing.assert_array_equal(g["T"], w["T"])


def test_registration_state_untouched(wm, drive):
    """A batched segmentation between set_target and icp_align, and between two aligns, leaves the registrations
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
    b.ground_segment_batch([S.rings_sensor_frame(130_000), S.rings_sensor_frame(60_000, 7)], keep=7)
    got = [b.icp_align(**kw)]
    b.ground_segment_batch(to_device(drive[:3]), G.load_yaml(S.YAML), keep=7, points=True)
    got.append(b.icp_align(**kw))
    b.close()
    for g, w in zip(got, want):
        assert g["rc"] == w["rc"] == 0
        np.testing.assert_array_equal(g["T"], w["T"])


def test_cap_too_small(ctx, wm, drive):
    import ctypes as C
    P = G.load_yaml(S.YAML)
    scans = drive[:3]
    good = ctx.ground_segment_batch(scans, P, keep=7)
    kept = sum(len(g[1]) for g in good)
    cap = kept // 2
    tab = (wm.GroundScan * 3)()
    for k, s in enumerate(scans):
        tab[k].pts, tab[k].n = s.ctypes.data, len(s)
    idx = np.full(cap + 16, -1, np.int32)
    offs = (C.c_size_t * 4)()
    p = wm.ground_params(P)
    rc = wm.lib().wm_ground_segment_batch(ctx._h, tab, 3, 12, wm.WM_MEM_HOST, C.byref(p), 7,
                                          C.c_void_p(idx.ctypes.data), cap, None, 0, wm.WM_MEM_HOST, offs, None, None,
                                          None)
    assert rc == wm.WM_ERR_ARG
    assert list(offs) == [0] + list(np.cumsum([len(g[1]) for g in good]))
    np.testing.assert_array_equal(idx[:cap], np.concatenate([g[1] for g in good])[:cap])
    assert (idx[cap:] == -1).all()
    later = ctx.ground_segment_batch(scans, P, keep=7)
    for g, w in zip(later, good):
        np.testing.assert_array_equal(g[0], w[0])
        np.testing.assert_array_equal(g[1], w[1])
        assert g[2] == w[2]


def test_no_scans(ctx):
    assert ctx.ground_segment_batch([]) == []
    res, kept, offs = ctx.ground_segment_batch([], points=True)
    assert res == [] and len(kept) == 0 and list(offs) == [0]
