"""The checker of the voxel-grid stress tests, checked: tests/voxel_reference.py's numpy restatement of
pcl::VoxelGrid<PointXYZ>::applyFilter against the C oracle (oracle/icp.c, wmo_voxel_grid) on every stress shape -- two
independent statements that must agree to the byte, the lattices of 2^32 cells and more included (the oracle's int
arithmetic wraps as the reference's mod-2^32 arithmetic does) -- and the generators held to what they claim, so that the
device tests reach the mechanisms they name."""
import numpy as np
import pytest

import voxel_reference as VR


@pytest.mark.parametrize("name", VR.NAMES)
def test_reference_equals_the_oracle(oracle, name):
    cloud, leaf, want = VR.shape(name)
    got = oracle.voxel_grid(cloud, leaf)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert VR.same_bytes(got, want), name  # bytes: the non-finite rows of an unfiltered cloud as well


def test_reference_on_a_case_small_enough_to_read():
    c = np.float32([[0.1, 0.1, 0.1], [1.5, 0.2, 0.3], [np.nan, 0, 0], [0.3, 0.5, 0.9], [-0.5, 0.5, 0.5], [0.2, np.inf, 0]])
    out = VR.voxel_grid(c, 1.0)  # leaves along x: -1, 0 (two points), 1
    assert out.tolist() == [[-0.5, 0.5, 0.5], [np.float32(0.4) / np.float32(2), np.float32(0.6) / np.float32(2), 0.5],
                            [1.5, np.float32(0.2), np.float32(0.3)]]
    assert VR.leaf_counts(c, 1.0).tolist() == [1, 2, 1]
    L = VR.lattice(c, 1.0)
    assert (L["n_valid"], L["extents"], L["div_b"], L["min_b"]) == (4, [3, 1, 1], [3, 1, 1], [-1, 0, 0])


def test_ladders_have_exactly_the_stated_leaf_sizes():
    cloud, leaf, want = VR.shape("ladder_wave")
    assert len(cloud) == 2299 and sorted(VR.leaf_counts(cloud, leaf)) == sorted(VR.LADDER)
    assert len(cloud) > VR.WAVE_AVG * len(want)  # the wave kernel
    L = VR.lattice(cloud, leaf)
    assert min(L["min_b"]) < 0 and all(a <= b for a, b in zip(L["div_b"], (11, 7, 5)))
    cloud, leaf, want = VR.shape("ladder_lane")
    assert len(cloud) == 2399 and sorted(VR.leaf_counts(cloud, leaf)) == sorted(VR.LADDER + [1] * VR.LADDER_PAD)
    assert len(cloud) <= VR.WAVE_AVG * len(want)  # the lane kernel
    # shuffled: the points of the largest leaf are not in a row
    key, _ = VR.keys(cloud, leaf)
    big = np.nonzero(key == np.bincount(key).argmax())[0]
    assert len(big) == 1000 and np.ptp(big) > 1500


def test_threshold_clouds_sit_on_the_threshold_and_one_past_it():
    cloud, leaf, want = VR.shape("threshold_at")
    L = VR.lattice(cloud, leaf)
    assert len(want) == 50 and L["n_valid"] == VR.WAVE_AVG * len(want) and len(cloud) == L["n_valid"] + 3
    assert (VR.leaf_counts(cloud, leaf) == VR.WAVE_AVG).all()
    cloud, leaf, want = VR.shape("threshold_past")
    assert len(want) == 50 and VR.lattice(cloud, leaf)["n_valid"] == VR.WAVE_AVG * len(want) + 1
    assert sorted(VR.leaf_counts(cloud, leaf)) == [VR.WAVE_AVG] * 49 + [VR.WAVE_AVG + 1]


def test_many_leaves_is_beyond_one_pass_of_everything():
    cloud, leaf, want = VR.shape("many_leaves")
    assert len(cloud) == 262500 > 256 << 10 and len(want) == 10500 > 2048 * 4
    assert (VR.leaf_counts(cloud, leaf) == 25).all() and len(cloud) > VR.WAVE_AVG * len(want)


def test_one_leaf_drifts_away_from_the_point():
    cloud, leaf, want = VR.shape("one_leaf")
    assert len(np.unique(cloud, axis=0)) == 1 and want.shape == (1, 3) and VR.lattice(cloud, leaf)["cells"] == 1
    assert (want[0] != cloud[0]).any()  # 5 000 sequential float additions: not the point itself
    tree = (cloud.astype(np.float64).sum(0) / len(cloud)).astype(np.float32)  # a sum in double, rounded once: the point
    assert np.array_equal(tree, cloud[0]) and not np.array_equal(tree, want[0])


def test_boundary_and_far_clouds():
    for leaf in (0.25, 0.1, 0.05):
        cloud, lf, want = VR.shape("boundaries_%g" % leaf)
        assert lf == leaf and len(cloud) == 3 * 81 * 11 * 6
        on = np.isin(cloud[:, 0], np.arange(-40, 41, dtype=np.float32) * np.float32(leaf))
        assert on.sum() == len(cloud) // 3  # a third exactly on k * leaf, the others one float off
        assert VR.lattice(cloud, leaf)["min_b"][0] in (-40, -41)
    for name, top in (("far_1e5", 2 ** 20), ("far_3e6", 2 ** 24)):
        cloud, leaf, want = VR.shape(name)
        L = VR.lattice(cloud, leaf)
        assert len(cloud) == 20000 and max(abs(b) for b in L["min_b"]) > top
        if name == "far_3e6":  # coordinates a quarter of a metre apart: points merge into far fewer leaves
            assert len(want) < len(VR.shape("far_1e5")[2])


def test_lattice_sizes_are_on_the_stated_side_of_the_rule():
    L = VR.lattice(*VR.shape("cube_1291")[:2])
    assert L["div_b"] == [1291] * 3 and L["cells"] == 2151685171 and 2 ** 31 <= L["cells"] < 2 ** 32 and not L["fires"]
    L = VR.lattice(*VR.shape("cube_past_the_rule")[:2])
    assert L["fires"] and L["cells"] < 2 ** 32
    cloud, leaf, want = VR.shape("cube_past_the_rule")
    assert VR.same_bytes(want, cloud) and not np.isfinite(cloud).all()
    L = VR.lattice(*VR.shape("flat")[:2])
    assert L["div_b"] == [46341, 46341, 2] and L["cells"] == 4294976562 >= 2 ** 32 and not L["fires"]
    assert L["extents"] == [46340, 46340, 1]
    cloud, leaf, want = VR.shape("flat")
    counts = VR.leaf_counts(cloud, leaf)
    assert len(cloud) == 3000 and (counts == 2).sum() >= 100 and L["n_valid"] == 2999 and len(want) == len(counts)
    L = VR.lattice(*VR.shape("column")[:2])
    assert L["div_b"][:2] == [2, 2] and L["cells"] == 4800000004 and not L["fires"]
    for name in ("cube_1291", "cube_past_the_rule", "column"):
        cloud = VR.shape(name)[0]
        assert 20 <= len(cloud) <= 60 and np.isnan(cloud).any() and np.isposinf(cloud).any() and np.isneginf(cloud).any()


def test_non_finite_shapes():
    for axis, name in enumerate(("holes_x", "holes_y", "holes_z")):
        cloud, leaf, want = VR.shape(name)
        bad = ~np.isfinite(cloud)
        assert bad[:, axis].sum() == 58 and bad.sum() == 58
        assert np.isnan(cloud).any() and np.isposinf(cloud).any() and np.isneginf(cloud).any()
    cloud, leaf, want = VR.shape("all_non_finite")
    assert len(want) == 0 and np.isfinite(cloud).any() and not np.isfinite(cloud).all(1).any()
    cloud, leaf, want = VR.shape("one_finite")
    assert VR.same_bytes(want, cloud[5:6])
