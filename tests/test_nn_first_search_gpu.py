"""How a query with nothing to start from finds its radius and its first candidate (k_nn_grid, csrc/wm_nn.hip: the
probe of the radius ladder's rungs for an empty box, and one point fetched from the first box that is not --
probe_box_empty in csrc/wm_nn_scan.hpp) changes the work, never the result: every case here
holds the grid search -- index AND d2 bits of every source point -- to the library's all-pairs search over the same
clouds, cold (every lane probes) and then twice warm after pose jumps (seeded lanes beside lanes that still have nothing).

The level-0 cell is forced (set_grid_cell); the ladder has a level more for every doubling of the cell below
0.2 max_corr, so max_corr chooses its depth.  The shapes are where a probe can go wrong: answers on every rung of the
ladder, above its top level and past the radius handed to the whole wave (12 cells); ladders of one level (nothing
coarse to probe on) up to the deepest; waves mixing lanes that stop on the first rung with lanes that climb; boxes that
hold points only beyond the radius or beyond the gate; targets of one and two points; queries outside the lattice, whose
coarse levels end in partial cells; gates below the neighbour distances; ties, NaNs and duplicates."""
import numpy as np
import pytest

from libwave_amd import synth

pytestmark = pytest.mark.gpu


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _same(got, want, what):
    gi, gd = got
    wi, wd = want
    bad = gi != wi
    assert not bad.any(), "%s: %d wrong indices (first at %d: got %d want %d)" % (
        what, bad.sum(), np.argmax(bad), gi[np.argmax(bad)], wi[np.argmax(bad)])
    keep = wi >= 0
    assert np.array_equal(gd[keep].view(np.uint32), wd[keep].view(np.uint32)), "%s: d2 bits differ" % what


def _searches(wm, ref, tgt, poses, max_corr, cell):
    """poses[0] cold, the others warm (seeded with the previous search's matches); returns the all-pairs answers."""
    ref, tgt = _f32(ref), _f32(tgt)
    b = wm.Context(0)
    try:
        b.set_source(ref)
        b.set_target(tgt)
        want = [b.nn_search(T, max_corr, wm.WM_NN_BRUTE) for T in poses]
    finally:
        b.close()
    c = wm.Context(0)
    try:
        c.set_grid_cell(cell)
        c.set_source(ref)
        c.set_target(tgt)
        for k, T in enumerate(poses):
            got = c.nn_search(T, max_corr, wm.WM_NN_GRID | (wm.WM_NN_WARM if k else 0))
            _same(got, want[k], "max_corr %g cell %g pose %d" % (max_corr, cell, k))
    finally:
        c.close()
    return want


def _jump():
    return [np.eye(4), synth.make_T((0.45, -0.3, 0.2), (0.0, 0.0, 0.0)), synth.make_T((0.1, 0.05, -0.4), (0.01, -0.02, 0.03))]


LIFTS = (0.3, 0.9, 1.7, 3.4, 6.8, 13.0, 20.0)


@pytest.mark.parametrize("max_corr", [1.0, 2.0, 4.0, 25.0])   # cell 0.25: ladders of 1, 2, 3 and kMaxLevels = 6 levels
def test_flat_target_source_lifted_onto_every_rung(wm, max_corr):
    """A sheet, and patches of the source lifted off it by 0.3 ... 20 cells, above and below: the answer falls on every
    rung (0.5, 1, 2, 4, 8 cells), above the top level's cell, and past the 12 cells at which a lane hands its query to
    the wave.  Under the smaller gates the higher patches end with no match."""
    rng = np.random.default_rng(41)
    cell = 0.25
    tgt = np.c_[rng.uniform(0, 14, (14000, 2)), np.zeros(14000)]
    tgt[0] = 0.0
    parts = []
    for k, lift in enumerate(LIFTS):
        for s, sign in enumerate((1.0, -1.0)):
            p = np.c_[rng.uniform(0.2, 1.8, (450, 2)) + [2.0 * k, 3.0 + 6.0 * s], np.full(450, sign * lift * cell)]
            parts.append(p + rng.normal(0, 0.01, p.shape))
    want = _searches(wm, np.concatenate(parts), tgt, _jump(), max_corr, cell)
    found = (want[0][0] >= 0).reshape(len(LIFTS), 2, 450).mean((1, 2))
    reach = np.array(LIFTS) * cell < max_corr - 0.05
    assert np.all(found[reach] == 1.0) and np.all(found[np.array(LIFTS) * cell > max_corr + 0.05] == 0.0), found


@pytest.mark.parametrize("n_far", [7, 8, 32, 57])
def test_one_wave_mixing_lanes_on_the_first_rung_and_lanes_that_climb(wm, n_far):
    """Blocks of 64 queries in far-apart octants (the source is processed in Morton order: a block is a wavefront), each
    an 8 x 8 lattice over its own pair of target sheets: the near lanes lie 0.1 cells above the lower sheet, the far
    ones 7 cells above it (and 7.4 below the upper one).  n_far = 32: alternately near and far; 7 / 8: either side of
    the layered walk's rule; 57: the near lanes are the few.  Far lanes walk level 1 while near lanes walk level 0."""
    rng = np.random.default_rng(43)
    cell = 0.1
    ref, tgt = [], [np.zeros((1, 3))]
    for b, corner in enumerate([(1.0, 1.0, 1.0), (21.0, 21.0, 21.0), (21.0, 1.0, 1.0)]):
        gx, gy = np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij")
        q = np.c_[gx.ravel() * 0.3, gy.ravel() * 0.3, np.zeros(64)] + corner + rng.uniform(-0.01, 0.01, (64, 3))
        far = np.zeros(64, bool)
        if n_far == 32:
            far[(np.arange(64) + b) % 2 == 1] = True
        else:
            far[rng.permutation(64)[:n_far]] = True
        q[:, 2] = corner[2] + np.where(far, 7.0, 0.1) * cell
        ref.append(q)
        for z in (0.0, 14.4 * cell):
            tgt.append(np.c_[rng.uniform(-0.6, 2.7, (2500, 2)) + corner[:2], np.full(2500, corner[2] + z)])
    want = _searches(wm, np.concatenate(ref), np.concatenate(tgt), _jump(), 1.1, cell)
    d0 = np.sqrt(want[0][1]) / cell
    assert ((d0 > 6.9) & (d0 < 7.2)).sum() == 3 * n_far and (d0 < 3.0).sum() == 3 * (64 - n_far), d0


def test_boxes_that_hold_points_only_beyond_the_radius_or_the_gate(wm):
    """Targets sit only on the diagonals of the queries' boxes: for the first cluster of queries 0.9 max_corr off along
    every axis (inside the box of the gate's radius, 1.56 max_corr away: the pass finds nothing it may keep, and the
    queries end without a match), for the second 0.5 max_corr off (inside the gate, but 1.7 times farther than the
    rung whose box first holds them: found, not certified, the radius grows).  Then a target of one point, and one of
    two points 40 cells apart."""
    rng = np.random.default_rng(47)
    cell, max_corr = 0.25, 2.0
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float)
    c1, c2 = np.array([5.0, 5.0, 5.0]), np.array([25.0, 5.0, 5.0])
    q1 = c1 + rng.uniform(-0.05, 0.05, (700, 3))
    q2 = c2 + rng.uniform(-0.05, 0.05, (700, 3))
    tgt = np.r_[np.zeros((1, 3)), c1 + corners * 0.9 * max_corr, c2 + corners * 0.5 * max_corr]
    poses = [np.eye(4), synth.make_T((0.05, -0.03, 0.02), (0, 0, 0)), synth.make_T((-0.02, 0.04, 0.01), (0.001, 0, 0))]
    want = _searches(wm, np.r_[q1, q2], tgt, poses, max_corr, cell)
    assert np.all(want[0][0][:700] < 0) and np.all(want[0][0][700:] >= 1)
    ref = rng.uniform(-3, 3, (1500, 3))                    # around the target's (last) point
    for pts in (np.array([[0.3, -0.2, 0.1]]), np.array([[0.0, 0.0, 0.0], [40 * cell, 0.0, 0.0]])):
        for mc in (1.0, 4.0):
            want = _searches(wm, ref + pts[-1], pts, _jump(), mc, cell)
            share = (want[0][0] >= 0).mean()
            assert 0.0 < share < 1.0, share


@pytest.mark.parametrize("max_corr", [1.0, 4.0])
def test_queries_outside_a_lattice_whose_every_level_ends_in_a_partial_cell(wm, max_corr):
    """Cell 0.25, target extent 4 x 8 x 2 with points on both end faces: 17 x 33 x 9 cells, and 9 x 17 x 5 and 5 x 9 x 3
    on the two coarser levels of max_corr 4 -- odd everywhere, so every coarse level's last cell is half a cell of the
    level below.  Queries lie beyond each face by less and by more than the top level's cell (1.0), and in the outer
    layers inside."""
    rng = np.random.default_rng(53)
    cell = 0.25
    ext = np.array([4.0, 8.0, 2.0])
    tgt = rng.uniform(0, 1, (9000, 3)) * ext
    tgt[0] = 0.0
    tgt[1] = ext
    for axis in range(3):                                       # a sprinkling exactly on the far faces: the last cells
        tgt[2 + 40 * axis:2 + 40 * (axis + 1), axis] = ext[axis]
    parts = [rng.uniform(0, 1, (1200, 3)) * ext]
    for axis in range(3):
        for side in (-1.0, 1.0):
            for dist in (0.1, 0.6, 1.7, 2.9):
                p = rng.uniform(0, 1, (140, 3)) * ext
                p[:, axis] = (ext[axis] + dist) if side > 0 else -dist
                parts.append(p)
            p = rng.uniform(0, 1, (200, 3)) * ext               # the outer layer inside
            p[:, axis] = (ext[axis] - rng.uniform(0, 0.12, 200)) if side > 0 else rng.uniform(0, 0.12, 200)
            parts.append(p)
    parts.append(rng.uniform(-2.5, 2.5, (600, 3)) + np.where(rng.random((600, 3)) < 0.5, 0.0, 1.0) * ext)  # the corners
    _searches(wm, np.concatenate(parts), tgt, _jump(), max_corr, cell)


@pytest.mark.parametrize("max_corr", [0.05, 0.3, 0.9])
def test_gate_below_some_neighbour_distances_with_nan_and_duplicate_targets(wm, max_corr):
    """Queries that end with no match have climbed the whole ladder, to the gate's radius, on empty boxes or on boxes
    whose points are all beyond the gate."""
    rng = np.random.default_rng(59)
    cell = 0.2
    base = rng.uniform(0, 5, (4000, 3))
    base[0] = 0.0
    tgt = np.r_[base, base[::-1], base[:500]]              # duplicates: the lowest index wins
    tgt[rng.permutation(len(tgt))[:300] + 1] = np.nan      # (the origin stays)
    tgt[5, 1] = np.inf
    ref = np.r_[base[rng.permutation(4000)[:3000]] + rng.normal(0, 0.03, (3000, 3)),
                rng.uniform(-1.5, 6.5, (3500, 3))]
    want = _searches(wm, ref, tgt, _jump(), max_corr, cell)
    share = (want[0][0] < 0).mean()
    assert 0.02 < share < 0.98, share


@pytest.mark.parametrize("cell", [0.125, 0.25, 1.0])
def test_exact_ties_on_a_shuffled_lattice_resolve_to_the_lowest_index(wm, cell):
    """Target: a lattice of multiples of 0.25 in shuffled order; queries at cell, face and edge centres: 8, 4 and 2
    targets at exactly the same float distance, whichever rung's pass meets them."""
    rng = np.random.default_rng(61)
    g = np.arange(0, 13, dtype=np.float32) * np.float32(0.25)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    tgt = np.r_[tgt[:1], tgt[1:][rng.permutation(len(tgt) - 1)]]      # (the origin stays a target point)
    c = np.stack(np.meshgrid(g[:-1], g[:-1], g[:-1], indexing="ij"), -1).reshape(-1, 3)
    ref = np.r_[c + np.float32(0.125), c + np.array([0.125, 0.125, 0.0], np.float32), c + np.array([0.125, 0.0, 0.0], np.float32)]
    poses = [np.eye(4), synth.make_T((0.25, 0.0, -0.25), (0, 0, 0)), synth.make_T((0.5, 0.5, 0.5), (0, 0, 0))]
    want = _searches(wm, ref, tgt, poses, 1.0, cell)
    n = len(c)
    d2 = want[0][1]
    assert np.all(d2[:n] == np.float32(3 * 0.125 ** 2)) and np.all(d2[n:2 * n] == np.float32(2 * 0.125 ** 2))
