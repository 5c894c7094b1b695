"""The target grid's counting sort by (y, z) rows (option grid_rows; counting_sort_rows, wm_grid.hip) against the sort by
cells it stands in for, and both against numpy.

A level is fetched as the search kernels read it (Context.debug_grid_level).  The reference is float32 numpy on the
geometry the fetch returns: floor((p - origin) * inv_h) per axis, clamped to the lattice; a bincount and its exclusive
sum are the expected cell_start, the original indices that fall in a cell its expected members.  Every case runs with
grid_rows = 2 (rows wherever structurally possible) and = 0 (never), with the cell size fixed by set_grid_cell and a
search radius of 6 cells, which leaves a ladder of exactly two levels: level 1 (derived from level 0) must satisfy the
same properties for the level-0 cells shifted right by one."""
import numpy as np
import pytest

from libwave_amd import synth

pytestmark = pytest.mark.gpu

NX_CAP = 4000  # kRowNxCap (wm_grid.hip): the longest row of cells the row-wise sort takes
NO_IDX = 0xFFFFFFFF


def _expected(g0, cloud, shift, dims):
    """(finite input indices, their cell index in the level `shift` above level 0, the level's cell_start)"""
    fin = np.flatnonzero(np.isfinite(cloud).all(axis=1))
    p = cloud[fin].astype(np.float32)
    c = np.floor((p - g0["origin"].astype(np.float32)) * np.float32(g0["inv_h"])).astype(np.int64)
    c = np.clip(c, 0, np.array(g0["dims"], np.int64) - 1) >> shift
    nx, ny, nz = dims
    cell = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    counts = np.bincount(cell, minlength=nx * ny * nz)
    start = np.zeros(nx * ny * nz + 1, np.int64)
    np.cumsum(counts, out=start[1:])
    return fin, cell, start


def _check_level(g0, g, cloud, shift, what):
    dims0 = g0["dims"]
    want_dims = tuple((d + (1 << shift) - 1) >> shift for d in dims0)
    assert g["dims"] == want_dims, (what, g["dims"], want_dims)
    fin, cell, start = _expected(g0, cloud, shift, g["dims"])
    assert g["cell_start"].shape == start.shape, what
    bad = g["cell_start"].astype(np.int64) != start
    assert not bad.any(), "%s: cell_start differs in %d of %d entries, first at %d" % (what, bad.sum(), bad.size, np.argmax(bad))
    n = len(fin)
    pts = g["pts"]
    assert pts.shape == (n + 4, 4), (what, pts.shape, n)
    idx = pts[:n, 3].copy().view(np.uint32).astype(np.int64)
    # every finite input point exactly once, no other
    assert np.array_equal(np.sort(idx), fin), "%s: the level's indices are not the finite input points, each once" % what
    assert np.array_equal(pts[:n, :3].copy().view(np.uint32), np.ascontiguousarray(cloud[idx]).view(np.uint32)), \
        "%s: coordinates not bit-identical to the input" % what
    cell_of_input = np.full(len(cloud), -1, np.int64)
    cell_of_input[fin] = cell
    c = cell_of_input[idx]
    j = np.arange(n)
    assert ((start[c] <= j) & (j < start[c + 1])).all(), "%s: a point lies outside its cell's run" % what
    assert np.isnan(pts[n:, :3]).all(), "%s: pad entries not NaN" % what
    assert (pts[n:, 3].copy().view(np.uint32) == NO_IDX).all(), "%s: pad entries without kNoIdx" % what


def _build(ctx, cloud, h, rows):
    ctx.set_option("grid_rows", rows)
    ctx.set_grid_cell(h)
    ctx.set_target(cloud)
    return ctx.debug_grid_level(0, 6.0 * h), ctx.debug_grid_level(1)


def _both_paths(ctx, cloud, h, dims=None):
    cloud = np.ascontiguousarray(cloud, np.float32)
    starts = {}
    for rows in (2, 0):
        g0, g1 = _build(ctx, cloud, h, rows)
        if dims is not None:
            assert g0["dims"] == dims, (g0["dims"], dims)
        assert g0["h"] == np.float32(h) and g1["h"] == np.float32(2 * h)
        _check_level(g0, g0, cloud, 0, "grid_rows=%d level 0" % rows)
        _check_level(g0, g1, cloud, 1, "grid_rows=%d level 1" % rows)
        starts[rows] = (g0["cell_start"], g1["cell_start"])
    for l in (0, 1):
        assert np.array_equal(starts[2][l], starts[0][l]), "level %d: the two paths' cell_start differ" % l
    return g0


def _span(rng, n, cells, h, extra=0.1):
    """n coordinates in [0, (cells - 1) h + extra], both ends among them: exactly `cells` cells of size h"""
    hi = (cells - 1) * h + (extra if cells > 1 else 0.1 * h)
    v = rng.uniform(0, hi, n)
    v[0], v[-1] = 0.0, hi
    return v


def _lattice_cloud(seed, n, dims, h):
    rng = np.random.default_rng(seed)
    c = np.stack([_span(rng, n, d, h) for d in dims], axis=1)
    c[1:-1] = c[1:-1][rng.permutation(n - 2)] if n > 2 else c[1:-1]
    return c.astype(np.float32)


@pytest.fixture()
def gctx(ctx):
    yield ctx
    ctx.set_option("grid_rows", 1)
    ctx.set_grid_cell(0.0)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_single_cell(gctx, n):
    rng = np.random.default_rng(n)
    cloud = rng.uniform(0, 0.1, (n, 3)).astype(np.float32)
    _both_paths(gctx, cloud, 0.5, dims=(1, 1, 1))


def test_one_row_only(gctx):
    _both_paths(gctx, _lattice_cloud(1, 5000, (300, 1, 1), 0.25), 0.25, dims=(300, 1, 1))


def test_one_column(gctx):
    """nx = 1 with 40 x 40 rows: the sort by cells under grid_rows = 1 (rows_apply), rows of one cell under 2"""
    cloud = _lattice_cloud(2, 4000, (1, 40, 40), 0.25)
    _both_paths(gctx, cloud, 0.25, dims=(1, 40, 40))
    g0, g1 = _build(gctx, cloud, 0.25, 1)
    _check_level(g0, g0, cloud, 0, "grid_rows=1 level 0")
    _check_level(g0, g1, cloud, 1, "grid_rows=1 level 1")


def test_all_points_in_one_of_many_rows(gctx):
    """70 000 points (more than 65 535) in ONE row of a 9 x 7 lattice of rows: the workgroup that gets it walks it
    alone.  Four more points span the lattice without touching its first or its last row, which stay empty."""
    rng = np.random.default_rng(3)
    h = 0.25
    row = np.stack([rng.uniform(0, 100 * h, 70000), np.full(70000, 4.5 * h), np.full(70000, 3.5 * h)], axis=1)
    span = np.array([[1.0, 0.0, 3.5 * h], [1.0, 8.5 * h, 3.5 * h], [1.0, 4.5 * h, 0.0], [1.0, 4.5 * h, 6.5 * h]])
    cloud = np.r_[row[:35000], span, row[35000:]].astype(np.float32)
    g0 = _both_paths(gctx, cloud, h)
    nx, ny, nz = g0["dims"]
    assert (ny, nz) == (9, 7)
    cs = g0["cell_start"]
    assert cs[nx] == 0 and cs[(ny * nz - 1) * nx] == cs[-1] == 70004  # first and last row empty


def test_corners_only(gctx):
    h = 0.25
    cloud = np.array([[x, y, z] for z in (0, 2.1 * h) for y in (0, 3.1 * h) for x in (0, 4.1 * h)], np.float32)
    g0 = _both_paths(gctx, cloud, h, dims=(5, 4, 3))
    assert np.count_nonzero(np.diff(g0["cell_start"].astype(np.int64))) == 8


def test_non_finite_points(gctx):
    rng = np.random.default_rng(4)
    cloud = rng.uniform(0, 5, (3001, 3)).astype(np.float32)
    bad = np.arange(0, 3001, 10)  # the first and the last element among them
    assert bad[-1] == 3000
    cloud[bad[0::3], 0] = np.nan
    cloud[bad[1::3], 1] = np.inf
    cloud[bad[2::3], 2] = -np.inf
    _both_paths(gctx, cloud, 0.25)


def test_a_single_finite_point(gctx):
    cloud = np.full((50, 3), np.nan, np.float32)
    cloud[17] = (1.0, -2.0, 3.0)
    _both_paths(gctx, cloud, 0.25, dims=(1, 1, 1))


@pytest.mark.parametrize("nx", [NX_CAP, NX_CAP + 1], ids=["at_cap", "cap_plus_1"])
def test_row_length_at_the_lds_cap(gctx, nx):
    """A long thin cloud whose rows are exactly as long as the finish kernel's LDS budget takes, and one cell longer
    (the sort by cells, whatever the option says)."""
    _both_paths(gctx, _lattice_cloud(5, 10000, (nx, 3, 3), 0.25), 0.25, dims=(nx, 3, 3))


def _expect_keys(oracle, ref, tgt, T, max_corr):
    moved = oracle.transform_cloud_f(ref, T.astype(np.float32))
    oi, od = oracle.KdTree(tgt).nn(moved)
    keep = od.astype(np.float64) <= float(max_corr) ** 2
    return np.where(keep, oi, -1), od, keep


def test_uniform_box_and_the_search_on_it(wm, gctx, oracle):
    """100 003 points, 2 500 rows: no multiple of a wave or a tile.  The search on either path's tables returns the exact
    kd-tree's keys, index and bits of d2 (as test_nn_prologue_gpu.py compares them)."""
    rng = np.random.default_rng(6)
    tgt = (rng.uniform(0, 1, (100003, 3)) * (30, 20, 5)).astype(np.float32)
    g0 = _both_paths(gctx, tgt, 0.2)
    assert g0["dims"][1] * g0["dims"][2] == 2500
    ref = (tgt[rng.permutation(len(tgt))[:20011]] + rng.normal(0, 0.05, (20011, 3))).astype(np.float32)
    T = synth.make_T((0.3, -0.2, 0.1), (0.02, -0.01, 0.04))
    max_corr = 1.2
    wi, wd, keep = _expect_keys(oracle, ref, tgt, T, max_corr)
    for rows in (2, 0):
        gctx.set_option("grid_rows", rows)
        gctx.set_grid_cell(0.2)
        gctx.set_source(ref)
        gctx.set_target(tgt)
        gi, gd = gctx.nn_search(T, max_corr, wm.WM_NN_GRID)
        assert np.array_equal(gi, wi), "grid_rows=%d: %d indices differ" % (rows, (gi != wi).sum())
        assert np.array_equal(gd[keep], wd[keep]), "grid_rows=%d: distances not bit-identical" % rows


def test_many_copies_of_one_point(gctx):
    rng = np.random.default_rng(7)
    cloud = np.r_[np.tile([[2.3, 1.7, 0.9]], (5000, 1)), rng.uniform(0, 5, (5000, 3))]
    _both_paths(gctx, cloud[rng.permutation(10000)], 0.25)


def test_points_on_cell_faces_and_on_the_box_maximum(gctx):
    """Coordinates that are exact multiples of the cell size from the origin (0), the largest among them the box's
    maximum: the last cell's upper face, which clamps into the last cell."""
    rng = np.random.default_rng(8)
    h = 0.25
    cloud = np.stack([rng.integers(0, 41, 6000), rng.integers(0, 25, 6000), rng.integers(0, 9, 6000)], axis=1) * h
    cloud[0], cloud[-1] = (0, 0, 0), (40 * h, 24 * h, 8 * h)
    off = rng.uniform(0, h, (6000, 3)) * (rng.random((6000, 3)) < 0.5)  # every other point: on some faces only
    off[::2] = 0
    off[-1] = 0
    cloud = np.minimum(cloud + off, cloud[-1])
    _both_paths(gctx, cloud, h, dims=(41, 25, 9))


def test_box_shifted_by_ten_kilometres(gctx):
    rng = np.random.default_rng(9)
    cloud = (rng.uniform(0, 1, (20000, 3)) * (20, 15, 4) + 1e4).astype(np.float32)
    _both_paths(gctx, cloud, 0.25)


def test_three_targets_in_turn_on_one_context(gctx):
    """big, small, big again: counters that were not put back, or a buffer sized by an earlier cloud, show in the third"""
    rng = np.random.default_rng(10)
    big = (rng.uniform(0, 1, (60001, 3)) * (25, 18, 4)).astype(np.float32)
    small = rng.uniform(0, 2, (501, 3)).astype(np.float32)
    again = (rng.uniform(0, 1, (59003, 3)) * (24, 19, 5)).astype(np.float32)
    for rows in (2, 1):
        for cloud in (big, small, again):
            g0, g1 = _build(gctx, cloud, 0.25, rows)
        _check_level(g0, g0, again, 0, "grid_rows=%d level 0" % rows)
        _check_level(g0, g1, again, 1, "grid_rows=%d level 1" % rows)
