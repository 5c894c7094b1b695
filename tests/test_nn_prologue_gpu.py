"""The start of a search wave (k_nn_grid, k_nn_cert): kernel arguments, then -- requested together -- the head run of
the state and the wave's streams, and only then the test of `done`.  The loads now run ahead of every test that used to
guard them, so: tail lanes read through clamped indices, a first search loads buffers it must not look at, a launch
queued behind `done` loads and must leave nothing behind, and the level ladder comes out of the kernel arguments at
every depth.  Every case is compared key for key (index and the bits of d2) with the oracle's exact kd-tree, as
test_nn_stress_gpu.py and test_cert_gpu.py do."""
import numpy as np
import pytest

from helpers import pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu


def _expect(oracle, ref, tgt, T, max_corr):
    moved = oracle.transform_cloud_f(ref, T.astype(np.float32))
    oi, od = oracle.KdTree(tgt).nn(moved)
    keep = od.astype(np.float64) <= float(max_corr) ** 2
    return np.where(keep, oi, -1), od, keep


def _same_keys(got, want, what=""):
    gi, gd = got
    wi, wd, keep = want
    bad = gi != wi
    assert not bad.any(), "%s: %d of %d indices differ (first at %d: got %d want %d)" % (
        what, bad.sum(), len(gi), np.argmax(bad), gi[np.argmax(bad)], wi[np.argmax(bad)])
    assert np.array_equal(gd[keep], wd[keep]), "%s: distances not bit-identical" % what


def _poses():
    return [synth.make_T((0.3, -0.2, 0.1), (0.02, -0.01, 0.04)),      # cold
            synth.make_T((0.25, -0.15, 0.08), (0.015, -0.01, 0.03)),  # warm, small step
            np.eye(4), np.eye(4)]                                     # warm jump, warm without motion


def _searches(wm, ctx, oracle, ref, tgt, max_corr):
    ctx.set_source(ref)
    ctx.set_target(tgt)
    for k, T in enumerate(_poses()):
        got = ctx.nn_search(T, max_corr, wm.WM_NN_GRID | (wm.WM_NN_WARM if k > 0 else 0))
        _same_keys(got, _expect(oracle, ref, tgt, T, max_corr), "pose %d" % k)


def _align_keys(wm, oracle, ref, tgt, K, max_corr, **opts):
    """A K-iteration align: its correspondences belong to the pose after K - 1 iterations (the same configuration
    run K - 1 iterations gives it: the path is bit-reproducible) and must be the kd-tree's under that pose."""
    out = []
    for iters in (K - 1, K):
        c = wm.Context(0)
        try:
            for k, v in opts.items():
                c.set_option(k, v)
            c.set_source(ref)
            c.set_target(tgt)
            r = c.icp_align(max_corr=max_corr, force_iterations=iters, nn_method=wm.WM_NN_GRID, carry_state=0)
            assert r["rc"] == 0, r
            r["corr"] = c.correspondences()
            out.append(r)
        finally:
            c.close()
    _same_keys(out[1]["corr"], _expect(oracle, ref, tgt, out[0]["T"], max_corr), "align")
    return out[1]


@pytest.fixture(scope="module")
def small_target():
    rng = np.random.default_rng(41)
    return rng.uniform(-3, 3, (3001, 3)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_source_sizes_around_one_wave(wm, ctx, oracle, small_target, n):
    """One lane, a wave less one, a full wave, a wave and one lane, three waves and a bit: the tail lanes load through
    indices clamped to n - 1 before anything is tested."""
    rng = np.random.default_rng(100 + n)
    ref = (small_target[rng.permutation(len(small_target))[:n]] + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    _searches(wm, ctx, oracle, ref, small_target, 1.0)
    if n >= 63:  # (a registration needs three correspondences) the certificate kernel's tail lanes, from iteration 1
        _align_keys(wm, oracle, ref, small_target, 5, 1.0, cert_from=1)


@pytest.mark.parametrize("cell,max_corr,levels", [(0.5, 1.0, 1), (0.05, 20.0, 6)], ids=["one_level", "six_levels"])
def test_ladder_depth_at_both_ends(wm, ctx, oracle, small_target, cell, max_corr, levels):
    """Cell sizes double per level until 0.2 max_corr is reached (ensure_levels): a cell of 0.5 with max_corr 1 leaves
    ONE level, a cell of 0.05 with max_corr 20 all SIX.  Queries far from the cloud climb the ladder."""
    h, L = cell, 1
    while h < 0.2 * max_corr and L < 6:
        h, L = 2 * h, L + 1
    assert L == levels
    rng = np.random.default_rng(43)
    near = small_target[:1500] + rng.normal(0, 0.05, (1500, 3))
    far = rng.uniform(-12, 12, (500, 3))
    ref = np.r_[near, far].astype(np.float32)
    ctx.set_grid_cell(cell)
    try:
        _searches(wm, ctx, oracle, ref, small_target, max_corr)
    finally:
        ctx.set_grid_cell(0.0)


def test_first_search_ignores_stale_keys_and_matches(wm, oracle):
    """A larger pair, then a smaller one on the same context with carry_state = 0: the second registration's first
    search loads the keys and matches the first one left before it knows that have_prev is 0.  It must not use
    them: the same transform, bit for bit, and the same correspondences as a fresh context's -- the kd-tree's."""
    big_r, big_t, _ = synth.pair(8000, seed=51, mode="resample")
    ref, tgt, _ = synth.pair(3000, seed=52, mode="resample")
    K = 6
    c = wm.Context(0)
    try:
        c.set_source(big_r)
        c.set_target(big_t)
        assert c.icp_align(max_corr=3.0, force_iterations=4, nn_method=wm.WM_NN_GRID, carry_state=0)["rc"] == 0
        c.set_source(ref)
        c.set_target(tgt)
        got = c.icp_align(max_corr=3.0, force_iterations=K, nn_method=wm.WM_NN_GRID, carry_state=0)
        got_corr = c.correspondences()
    finally:
        c.close()
    fresh = _align_keys(wm, oracle, ref, tgt, K, 3.0)
    assert got["rc"] == 0
    assert np.array_equal(got["T"], fresh["T"])
    assert np.array_equal(got_corr[0], fresh["corr"][0]) and np.array_equal(got_corr[1], fresh["corr"][1])


def test_launches_queued_behind_done_leave_nothing(wm, oracle):
    """A free-running registration (PCL's stopping rules, max_iter far above where it stops): the host runs ahead of
    the device, so searches are queued behind the `done` the solve sets.  They load, and must store nothing and add
    nothing: the oracle's iteration count, state and transform (the bounds of test_icp_gpu.py's free-running case),
    and the correspondences of the last executed search -- the kd-tree's under the pose before the last step."""
    ref, tgt, _ = synth.pair(10000, seed=8, mode="resample")
    c = wm.Context(0)
    try:
        c.set_source(ref)
        c.set_target(tgt)
        got = c.icp_align(max_corr=3.0, max_iter=400, nn_method=wm.WM_NN_GRID, carry_state=0)
        got_corr = c.correspondences()
    finally:
        c.close()
    want = oracle.icp_align(ref, tgt, max_corr=3.0, max_iter=400, incremental_float=0)
    assert got["rc"] == 0 and got["converged"]
    assert (got["iterations"], got["state"]) == (want["iterations"], want["state"])
    assert got["iterations"] < 100
    dt, ang = pose_error(got["T"], want["T"])
    assert dt <= 1e-7 and ang <= 1e-8, (dt, ang)
    c = wm.Context(0)
    try:
        c.set_source(ref)
        c.set_target(tgt)
        before = c.icp_align(max_corr=3.0, force_iterations=got["iterations"] - 1, nn_method=wm.WM_NN_GRID, carry_state=0)
    finally:
        c.close()
    _same_keys(got_corr, _expect(oracle, ref, tgt, before["T"], 3.0), "free-running")


def test_one_rank_sharded_path_reads_its_slab_from_the_head_run(wm, oracle, monkeypatch):
    """WM_SHARD_FORCE = 1: a one-rank group runs the sharded loop, whose searches test every query against
    slab_on / slab_lo / slab_hi.  The unsharded registration's transform (they differ by summation order only: the
    bound of test_shard_product_gpu.py), whose own correspondences are the kd-tree's."""
    monkeypatch.setenv("WM_SHARD_FORCE", "1")
    ref, tgt, _ = synth.pair(20000, seed=3)
    K = 6
    want = _align_keys(wm, oracle, ref, tgt, K, 3.0)
    comm = wm.Comm.init_rank(0, wm.Comm.unique_id(), 0, 1)
    c = wm.Context(0)
    try:
        got = c.icp_align_sharded(comm, ref, tgt, max_corr=3.0, force_iterations=K, nn_method=wm.WM_NN_GRID)
    finally:
        c.close()
        comm.close()
    assert got["rc"] == 0 and got["rccl_ranks"] == 1 and got["owned_violations"] == 0
    assert (got["iterations"], got["n_corr"]) == (want["iterations"], want["n_corr"])
    dt, ang = pose_error(got["T"], want["T"])
    assert dt <= 1e-9 and ang <= 1e-9, (dt, ang)


def test_certificate_kernel_from_iteration_one_small_pair(wm, oracle):
    ref, tgt, _ = synth.pair(3000, seed=61, mode="resample")
    K = 10
    r = _align_keys(wm, oracle, ref, tgt, K, 3.0, cert_from=1)
    assert r["cert_launches"] == K - 1
