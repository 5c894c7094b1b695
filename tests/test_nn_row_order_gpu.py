"""The order in which the grid search visits the (y,z) rows of a box (scan_box_bal, csrc/wm_nn_scan.hpp; the walk's
arithmetic: csrc/wm_zigzag.hpp) changes the work, never the result: every case here holds the grid search -- index AND
d2 bits of every source point -- to the library's all-pairs search over the same clouds.  Through the C ABI: unseeded
searches (one cold search), seeded ones (a warm search; a forced-iterations align and its correspondences), far seeds (a warm search
after a pose jump) and the certificate kernel's searches.

The level-0 cell is forced (set_grid_cell) so that boxes get the wanted number of rows: the target's lower corner is the
lattice's origin, so with a cell of 2^-k and a target that has a point at the origin the cell faces are exact floats.
The shapes are where a nearest-first walk with an early stop can go wrong: one side of the walk empty from the start
(flat targets, queries outside the lattice), boxes of even and odd width, queries exactly on cell faces (non-positive
margins), exact ties (the lowest index must win whatever is seen first), waves that mix lanes with big boxes and lanes
with small ones on either side of the layered walk's rule (8 lanes with more than 18 rows) and on two grid levels, NaN
and duplicate targets, and gates below some neighbour distances."""
import numpy as np
import pytest

from libwave_amd import synth

pytestmark = pytest.mark.gpu


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _brute(wm, ref, tgt, T, max_corr):
    c = wm.Context(0)
    try:
        c.set_source(ref)
        c.set_target(tgt)
        return c.nn_search(T, max_corr, wm.WM_NN_BRUTE)
    finally:
        c.close()


def _same(got, want, what):
    gi, gd = got
    wi, wd = want
    bad = gi != wi
    assert not bad.any(), "%s: %d wrong indices (first at %d: got %d want %d)" % (
        what, bad.sum(), np.argmax(bad), gi[np.argmax(bad)], wi[np.argmax(bad)])
    keep = wi >= 0
    assert np.array_equal(gd[keep].view(np.uint32), wd[keep].view(np.uint32)), "%s: d2 bits differ" % what


def _searches(wm, ref, tgt, poses, max_corr, cell):
    """poses[0] cold, the others warm (seeded with the previous search's matches)."""
    ref, tgt = _f32(ref), _f32(tgt)
    want = [_brute(wm, ref, tgt, T, max_corr) for T in poses]
    c = wm.Context(0)
    try:
        c.set_grid_cell(cell)
        c.set_source(ref)
        c.set_target(tgt)
        for k, T in enumerate(poses):
            got = c.nn_search(T, max_corr, wm.WM_NN_GRID | (wm.WM_NN_WARM if k else 0))
            _same(got, want[k], "pose %d" % k)
    finally:
        c.close()
    return want


def _jump():
    return [np.eye(4), synth.make_T((0.45, -0.3, 0.2), (0.0, 0.0, 0.0)), synth.make_T((0.1, 0.05, -0.4), (0.01, -0.02, 0.03)),
            np.eye(4)]


@pytest.mark.parametrize("lift_cells", [0.4, 2.3, 7.6])
def test_flat_target_source_lifted_by_a_fraction_of_cells(wm, lift_cells):
    """One z layer: the start layer clamps to it and one direction of the walk is empty from the first step."""
    rng = np.random.default_rng(11)
    cell = 0.25
    tgt = np.c_[rng.uniform(0, 12, (12000, 2)), np.zeros(12000)]
    tgt[0] = 0.0
    ref = tgt[rng.permutation(len(tgt))[:6000]] + np.r_[rng.normal(0, 0.05, 2), 0] + [0, 0, lift_cells * cell]
    for sign in (1.0, -1.0):   # above and below the layer
        _searches(wm, ref * [1, 1, sign], tgt, _jump(), 3.0, cell)


@pytest.mark.parametrize("cell", [0.25, 0.5])
def test_queries_outside_the_lattice_on_each_side_and_in_its_outer_layers(wm, cell):
    rng = np.random.default_rng(13)
    tgt = rng.uniform(0, 4, (8000, 3))
    tgt[0] = 0.0
    parts = [rng.uniform(0, 4, (1500, 3)),                      # inside
             rng.uniform(0, 4, (600, 3)) * [1, 1, 0.05],        # first layers / rows of every axis ...
             rng.uniform(0, 4, (600, 3)) * [1, 0.05, 1],
             rng.uniform(0, 4, (600, 3)) * [0.05, 1, 1]]
    parts += [4.0 - p for p in parts[1:]]                       # ... and the last
    for axis in range(3):
        for side in (-1.0, 1.0):
            for dist in (0.1, 0.6, 1.4, 2.9):                   # beyond the face by less and by more than the radii
                p = rng.uniform(0, 4, (150, 3))
                p[:, axis] = (4.0 + dist) if side > 0 else -dist
                parts.append(p)
    _searches(wm, np.concatenate(parts), tgt, _jump(), 1.5, cell)


def test_even_and_odd_boxes_and_queries_exactly_on_cell_faces(wm):
    """Queries on a lattice of half cells: every combination of `on a face` / `in the middle` per axis, so fy and fz are
    integers for a quarter of them (margin <= 0: the radius must grow), and the boxes' widths alternate."""
    rng = np.random.default_rng(17)
    cell = 0.25
    tgt = rng.uniform(0, 3, (9000, 3))
    tgt[0] = 0.0
    g = np.arange(0, 25, dtype=np.float32) * np.float32(0.125)
    ref = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    ref = ref[rng.permutation(len(ref))[:9000]]
    poses = [np.eye(4), synth.make_T((0.25, -0.5, 0.75), (0, 0, 0)), synth.make_T((0.125, 0.125, 0.125), (0, 0, 0)), np.eye(4)]
    _searches(wm, ref, tgt, poses, 2.0, cell)


@pytest.mark.parametrize("cell", [0.125, 0.25, 1.0])
def test_exact_ties_resolve_to_the_lowest_index_in_any_order(wm, cell):
    """Target: a lattice of multiples of 0.25 in shuffled order; queries at cell, face and edge centres: 8, 4 and 2
    targets at exactly the same float distance."""
    rng = np.random.default_rng(19)
    g = np.arange(0, 14, dtype=np.float32) * np.float32(0.25)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    tgt = np.r_[tgt[:1], tgt[1:][rng.permutation(len(tgt) - 1)]]      # (the origin stays a target point)
    c = np.stack(np.meshgrid(g[:-1], g[:-1], g[:-1], indexing="ij"), -1).reshape(-1, 3)
    ref = np.r_[c + np.float32(0.125), c + np.array([0.125, 0.125, 0.0], np.float32), c + np.array([0.125, 0.0, 0.0], np.float32)]
    poses = [np.eye(4), synth.make_T((0.25, 0.0, -0.25), (0, 0, 0)), synth.make_T((0.5, 0.5, 0.5), (0, 0, 0)), np.eye(4)]
    want = _searches(wm, ref, tgt, poses, 1.0, cell)
    n = len(c)
    d2 = want[0][1]
    assert np.all(d2[:n] == np.float32(3 * 0.125 ** 2)) and np.all(d2[n:2 * n] == np.float32(2 * 0.125 ** 2))


def test_waves_mixing_big_boxes_and_small_ones(wm):
    """Three blocks of 64 queries, far apart (the source is processed in Morton order: a block is a wavefront).  In
    the second search every query is seeded with its first match: for a `far` lane that is a target point that was
    on top of it before the pose jumped by 0.4 m (radius 0.4 m = 4 cells: a box of 9 x 9 rows, more than the 18 of the
    layered walk's rule), for a `near` lane a target point placed where the jump takes the query (a box of 1-4 rows).
    Block A has exactly 7 far lanes, block B exactly 8 (either side of the rule's 8 lanes); block C's far lanes were
    matched 0.4 m AGAINST the jump, so their seeds are 0.8 m away: they scan level 1 while its near lanes scan level 0."""
    rng = np.random.default_rng(23)
    cell = 0.1
    t = np.array([0.4, 0.0, 0.0])
    lat = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 3) * 2.0
    ref, tgt = [], [np.zeros((1, 3))]
    for corner, n_far, back in [((1.0, 1.0, 1.0), 7, False), ((17.0, 17.0, 17.0), 8, False), ((33.0, 1.0, 1.0), 12, True)]:
        q = lat + corner + rng.uniform(-0.02, 0.02, lat.shape)
        far = np.zeros(64, bool)
        far[rng.permutation(64)[:n_far]] = True
        first = np.where(far[:, None], q - t if back else q, q + t + rng.normal(0, 0.004, q.shape))
        ref.append(q)
        tgt.append(first)
        # something for the far lanes to find in the second search, 0.15-0.3 m from where the jump takes them (and
        # on the far side of it: more than 0.4 m from where they are in the first)
        v = rng.normal(size=(64, 3))
        v[:, 0] = np.abs(v[:, 0])
        tgt.append((q + t + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.15, 0.3, (64, 1)))[far])
    ref, tgt = _f32(np.concatenate(ref)), _f32(np.concatenate(tgt))
    T = np.eye(4)
    T[:3, 3] = t
    want = _searches(wm, ref, tgt, [np.eye(4), T, np.eye(4)], 1.1, cell)
    # the construction holds: in the first search every lane found its planted point, at the planted distance
    d0 = np.sqrt(want[0][1])
    assert (d0[:64] < 0.01).sum() == 7 and (d0[64:128] < 0.01).sum() == 8
    assert (np.abs(d0 - 0.4) < 0.02).sum() == 192 - 15


def test_nan_and_duplicate_targets_and_a_gate_below_some_neighbour_distances(wm):
    rng = np.random.default_rng(29)
    cell = 0.2
    base = rng.uniform(0, 5, (4000, 3))
    base[0] = 0.0
    tgt = np.r_[base, base[::-1], base[:500]]              # duplicates: the lowest index wins
    tgt[rng.permutation(len(tgt))[:300] + 1] = np.nan      # (the origin stays)
    tgt[5, 1] = np.inf
    ref = np.r_[base[rng.permutation(4000)[:3000]] + rng.normal(0, 0.03, (3000, 3)),
                rng.uniform(-1, 6, (3000, 3))]
    for max_corr in (0.05, 0.3):                           # below many / some neighbour distances: no match stays none
        want = _searches(wm, ref, tgt, _jump(), max_corr, cell)
        share = (want[0][0] < 0).mean()
        assert 0.02 < share < 0.98, share


def _align(wm, ref, tgt, iters, cell, max_corr, **opts):
    c = wm.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        c.set_grid_cell(cell)
        c.cert_log(16)
        c.set_source(ref)
        c.set_target(tgt)
        r = c.icp_align(max_corr=max_corr, force_iterations=iters, nn_method=wm.WM_NN_GRID, carry_state=0)
        r["corr"] = c.correspondences()
        r["cert_log"] = c.cert_log()
        return r
    finally:
        c.close()


@pytest.mark.parametrize("cell", [0.08, 0.3])
def test_seeded_searches_of_an_align_leave_the_all_pairs_correspondences(wm, cell):
    """A K-iteration align leaves the matches of its last search, made under the pose after K - 1 iterations; the early
    iterations' seeds are a few cells off (cell 0.08: boxes of dozens of rows, the layered walk; 0.3: the cursor)."""
    ref, tgt, _ = synth.pair(16000, seed=31, mode="resample")
    K = 5
    prev = _align(wm, ref, tgt, K - 1, cell, 3.0, cert_from=-2)
    want = _brute(wm, _f32(ref), _f32(tgt), prev["T"], 3.0)
    r = _align(wm, ref, tgt, K, cell, 3.0, cert_from=-2)
    assert r["rc"] == 0 and r["cert_launches"] == 0
    _same(r["corr"], want, "cell %.2f" % cell)


@pytest.mark.parametrize("cell", [0.08, 0.3])
def test_certificate_launch_after_a_large_step_equals_a_full_search(wm, cell):
    """cert_from = 1: iteration 0 searches, iterations 1.. are certificate launches; the first steps of a registration
    are large, so a real share of the queries fails the proof and is searched by k_nn_cert (with runner-up tracking).
    What is left must be a full search's correspondences."""
    ref, tgt, _ = synth.pair(16000, seed=37, mode="resample")
    K = 4
    prev = _align(wm, ref, tgt, K - 1, cell, 3.0, cert_from=-2)
    want = _brute(wm, _f32(ref), _f32(tgt), prev["T"], 3.0)
    r = _align(wm, ref, tgt, K, cell, 3.0, cert_from=1)
    assert r["rc"] == 0 and r["cert_launches"] == K - 1
    log = np.asarray(r["cert_log"])
    # the first launch has no bounds yet and searches everything; in the later ones some queries settle and some
    # fail the proof (measured on this pair: 9 255 and 9 818 of 16 000 are searched)
    assert len(log) == K - 1 and log[0] == len(ref), log
    assert np.all(log[1:] > 0) and np.all(log[1:] < len(ref)), log
    _same(r["corr"], want, "cell %.2f" % cell)
