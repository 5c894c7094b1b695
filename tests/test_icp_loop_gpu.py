"""The host side of the ICP iteration loop (icp_run_loop, csrc/wm_icp.hip): it runs `lag` iterations ahead of the
device, waits for the records the solve kernels publish (host_wait: spin, yield after `spin_us`, then block), and with
`profile` on keeps a pool of events around every launch.  None of that may touch the registration: how far the host
runs ahead moves which iterations certify -- the sums then differ in order only --, and how it waits or whether it
times changes nothing at all."""
import numpy as np
import pytest

from helpers import pose_error
from libwave_amd import synth

pytestmark = pytest.mark.gpu

FREE = dict(max_iter=60, t_eps=1e-12, fit_eps=1e-9)


@pytest.fixture(scope="module")
def pair():
    ref, tgt, _ = synth.pair(30000, seed=15, mode="resample")
    return ref, tgt


def _align(wm, pair, opts, **kw):
    c = wm.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        c.set_source(pair[0])
        c.set_target(pair[1])
        r = c.icp_align(max_corr=3.0, nn_method=wm.WM_NN_GRID, carry_state=0, **kw)
        r["times"] = c.iteration_times()
        return r
    finally:
        c.close()


def _same_bits(a, b):
    assert a["rc"] == 0 and b["rc"] == 0
    assert np.array_equal(a["T"], b["T"])
    assert a["iterations"] == b["iterations"] and a["state"] == b["state"] and a["n_corr"] == b["n_corr"]
    assert a["cert_launches"] == b["cert_launches"] and a["late_iterations"] == b["late_iterations"]


def test_free_running_align_does_not_depend_on_the_lag(wm, pair):
    """The loop ends on a `done` seen while the host is ahead: same stop, same registration for every lag."""
    res = [_align(wm, pair, {"lag": lag}, **FREE) for lag in (1, 2, 4)]
    for r in res:
        assert r["rc"] == 0
        assert r["iterations"] == res[0]["iterations"] and r["state"] == res[0]["state"]
        dt, da = pose_error(r["T"], res[0]["T"])
        print("lag: iterations %d, cert_launches %d, dt %.3e, da %.3e" % (r["iterations"], r["cert_launches"], dt, da))
        assert dt < 1e-9 and da < 1e-10, (dt, da)  # the sums differ in order only


def test_how_long_the_host_spins_changes_nothing(wm, pair):
    a = _align(wm, pair, {"lag": 2, "spin_us": 0}, **FREE)
    b = _align(wm, pair, {"lag": 2, "spin_us": 80}, **FREE)
    _same_bits(a, b)


def test_forced_iterations_for_every_lag(wm, pair):
    for lag in (1, 2, 4):
        r = _align(wm, pair, {"lag": lag}, force_iterations=20)
        assert r["rc"] == 0 and r["iterations"] == 20, (lag, r["iterations"])


def test_the_wait_for_the_resident_kernel(wm, pair):
    a = _align(wm, pair, {"late": 1, "spin_us": 0}, **FREE)
    b = _align(wm, pair, {"late": 1, "spin_us": 80}, **FREE)
    _same_bits(a, b)
    assert a["late_iterations"] > 0


@pytest.mark.parametrize("late", [0, 1])
def test_profiling_does_not_touch_the_work(wm, pair, late):
    plain = _align(wm, pair, {"late": late}, profile=0, **FREE)
    timed = _align(wm, pair, {"late": late}, profile=2, **FREE)
    _same_bits(plain, timed)
    if timed["state"] not in ("NO_CORRESPONDENCES", "DEGENERATE"):
        assert timed["nn_launches"] + timed["late_iterations"] == timed["iterations"]
    assert len(timed["times"]) > 0
    assert all(t == -1.0 or t >= 0.0 for t in timed["times"]), timed["times"]
