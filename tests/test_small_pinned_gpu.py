"""wm_icp_batch_match and the one-pair path's statistics and LUMold kernels against tests/golden/small_icp_bits.json,
bit for bit: the record of what the library returned before k_icp_small was cut into named steps and the iteration's
sums, LUMold's sums and normal matrix, and PCL's float transform came to have one definition each
(tests/golden/make_golden_small.py has the inputs and what is kept of an output).  test_batch_gpu.py holds the small
path to the oracle and to the one-pair path within 1e-7 ... 1e-9; a term that lands in another chunk row, rows added in
another order, or a term formed in float where it was formed in double moves less than that and is seen here alone."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_small as G  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(rec, want, src, tgt, what):
    for k, v in G.clouds_digest(src, tgt).items():
        assert v == want[k], "%s: the input is not the recorded one (%s)" % (what, k)
    for k, v in rec.items():
        assert v == want[k], (what, k, v, want[k])


def test_the_record_holds_every_input():
    want = G.load()
    ids = [what for _, _, items in G.inputs() for what, _, _ in items] + [what for what, _, _ in G.one_pair_inputs()]
    assert sorted(want) == sorted(ids) and len(want) == 30
    for what, r in want.items():
        if what.startswith("15/"):
            assert r["match"]["rc"] == 0 and r["match_trimmed"]["rc"] == 0
        elif int(what.split("/")[0]) not in (7, 8, 9):
            assert r["rc"] == 0 and r["n_corr"] >= 3 and r["T"] is not None, what
            assert (r["info"] is None) == what.endswith("noinfo")


def test_one_call_per_parameter_set_returns_the_recorded_bits(wm, ctx):
    """targets in LDS and targets in HBM scratch in one call: two launches, and small_run's permutation of the rows"""
    want = G.load()
    for name, kw, items in G.inputs():
        got = ctx.icp_batch_match([(s, t) for _, s, t in items], **kw)
        assert len(got) == len(items)
        for (what, s, t), g in zip(items, got):
            _same(G.digest(g), want[what], s, t, "%s in a call of %d" % (what, len(items)))


def test_a_call_per_item_returns_the_recorded_bits(wm, ctx):
    want = G.load()
    for name, kw, items in G.inputs():
        for what, s, t in items:
            _same(G.digest(ctx.icp_batch_match([(s, t)], **kw)[0]), want[what], s, t, what + " alone")


def test_the_one_pair_path_returns_the_recorded_bits(wm, ctx):
    want = G.load()
    for what, s, t in G.one_pair_inputs():
        _same(G.one_pair(ctx, s, t), want[what], s, t, what)
