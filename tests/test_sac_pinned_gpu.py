"""wm_sac_segment and wm_sac_segment_batch WITH THE REFIT against tests/golden/sac_refit_bits.json, bit for bit: the
record of what the library returned before the two entry points came to share one set of kernels and one host back
(tests/golden/make_golden_sac.py has the inputs and what is kept of an output).  test_sac_gpu.py holds the refit to
bounds and test_sac_batch_gpu.py holds a batch to the single call; a change to which wave feeds which bin of the refit's
sums, or to the order the bins are added in, moves both alike and is seen here alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_sac as G  # noqa: E402

pytestmark = pytest.mark.gpu

_IN = None


def _inputs():
    global _IN
    if _IN is None:
        _IN = G.inputs()
        for _, P, _ in _IN:
            P.setflags(write=False)
    return _IN


def _host(got):
    return {k: v if v is None or isinstance(v, (int, float, np.ndarray)) else v.cpu().numpy() for k, v in got.items()}


def _key(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))


def _same(got, want, P, what):
    assert G._sha(P) == want["input_sha256"] and len(P) == want["n"], "%s: the input is not the recorded one" % what
    rec = G.digest(_host(got))
    for k, v in rec.items():
        assert v == want[k], (what, k, v, want[k])


def test_the_record_holds_every_input():
    want = G.load()
    assert sorted(want) == sorted(what for what, _, _ in _inputs()) and len(want) == 23
    assert sum(r["refined"] for r in want.values()) >= 15  # (the record is of the refit)


def test_the_single_call_returns_the_recorded_bits(wm, ctx):
    want = G.load()
    for what, P, kw in _inputs():
        _same(ctx.sac_segment(P, **kw), want[what], P, what)


def test_batches_return_the_recorded_bits(wm, ctx):
    """one batch per set of parameters, the scans in the record's order"""
    want = G.load()
    groups = {}
    for what, P, kw in _inputs():
        groups.setdefault(_key(kw), (kw, []))[1].append((what, P))
    assert len(groups) == 9
    for kw, scans in groups.values():
        batch = ctx.sac_segment_batch([P for _, P in scans], **kw)
        for (what, P), got in zip(scans, batch):
            assert got["batch_rc"] == wm.WM_OK
            _same(got, want[what], P, "%s in a batch of %d" % (what, len(scans)))
