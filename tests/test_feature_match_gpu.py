"""wm_feature_match (libwave_amd/csrc/wm_feature_match.hip) on the GPU: idx and d2 bit-equal to the numpy float32
restatement (tests/fpfh_reference.py: match -- a loop over the 33 bins, vectorised over pairs).  Sizes around the
kernel's shapes: a wave (64), a tile of B (128 rows), the rows of A a workgroup holds (512)."""
import numpy as np
import pytest

import fpfh_reference as FR

pytestmark = pytest.mark.gpu

TILE = 128
SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]


@pytest.fixture(scope="module")
def dev(wm):
    c = wm.Context(0)  # (no clouds are ever set on it)
    yield c
    c.close()


def rows(n, seed, width=33):
    """descriptor-like rows: a few occupied bins out of 33, values on a coarse lattice so that equal distances occur"""
    rng = np.random.default_rng(seed)
    r = np.float32(rng.integers(0, 40, (n, width)) * 2.5) * (rng.random((n, width)) < 0.4)
    r[:, 0] += 1  # (no accidental zero row)
    return np.ascontiguousarray(r, np.float32)


def same(got, want):
    idx, d2 = want
    assert np.array_equal(got["idx"], idx)
    assert np.array_equal(np.asarray(got["d2"]).view(np.uint32), d2.view(np.uint32))
    assert got["n_matched"] == int((idx >= 0).sum())


@pytest.mark.parametrize("na", SIZES + [513])
def test_sizes_plain_and_reciprocal(dev, na):
    a = rows(na, na)
    for nb in SIZES:
        b = rows(nb, 1000 + nb)
        same(dev.feature_match(a, b), FR.match(a, b))
        same(dev.feature_match(a, b, reciprocal=True), FR.match(a, b, reciprocal=True))


def test_ties_take_the_lowest_index_and_zero_rows_match_nothing(dev):
    a = rows(200, 1)
    b = rows(300, 2)
    b[150:160] = b[3]   # duplicates of row 3, and of what a's rows are nearest to
    b[10:20] = a[5]
    a[7] = 0
    a[64] = 0
    b[0] = 0
    b[299] = 0
    b[130] = a[9]
    b[0, :] = 0
    for recip in (False, True):
        got = dev.feature_match(a, b, reciprocal=recip)
        same(got, FR.match(a, b, reciprocal=recip))
        assert got["idx"][7] == -1 and got["idx"][64] == -1 and got["d2"][7] == 0
        assert 0 not in got["idx"] and 299 not in got["idx"]
    plain = dev.feature_match(a, b)
    assert plain["idx"][5] == 10 and plain["d2"][5] == 0 and plain["idx"][9] == 130
    # nothing but zero rows, and no rows at all, on B's side
    assert np.all(dev.feature_match(a, np.zeros((5, 33), np.float32))["idx"] == -1)
    none = dev.feature_match(a, np.zeros((0, 33), np.float32), reciprocal=True)
    assert np.all(none["idx"] == -1) and none["n_matched"] == 0


def test_strides_and_memory_spaces(dev):
    import torch
    a36, b36 = rows(300, 3, width=36), rows(450, 4, width=36)  # the three floats behind a row are the caller's
    a36[11, :33] = 0
    b36[17, :33] = 0
    a, b = np.ascontiguousarray(a36[:, :33]), np.ascontiguousarray(b36[:, :33])
    for recip in (False, True):
        want = FR.match(a, b, reciprocal=recip)
        same(dev.feature_match(a, b, reciprocal=recip), want)
        same(dev.feature_match(a36, b36, reciprocal=recip), want)
        got = dev.feature_match(torch.from_numpy(a36).cuda(), torch.from_numpy(b36).cuda(), reciprocal=recip)
        same(dict(idx=got["idx"].cpu().numpy(), d2=got["d2"].cpu().numpy(), n_matched=got["n_matched"]), want)


def test_descriptors_of_two_clouds(dev, wm):
    c = wm.Context(0)
    desc = []
    for name, n in (("scan", 2000), ("scene", 3000)):
        cloud = FR.clouds()[name][:n]
        c.set_source(cloud)
        c.set_target(cloud)
        desc.append(c.fpfh(1)["fpfh"])
    c.close()
    for recip in (False, True):
        same(dev.feature_match(desc[0], desc[1], reciprocal=recip), FR.match(desc[0], desc[1], reciprocal=recip))
    me = dev.feature_match(desc[0], desc[0])  # a set against itself: every row finds itself, or an equal row before it
    valid = np.any(desc[0] != 0, axis=1)
    own = np.arange(len(desc[0]))
    assert np.all(me["d2"] == 0) and np.all(me["idx"][valid] >= 0) and np.all(me["idx"] <= own)
    assert np.array_equal(desc[0][me["idx"][valid]], desc[0][valid]) and np.all(me["idx"][~valid] == -1)


def test_argument_errors(dev, wm):
    a = rows(4, 1, width=36)
    with pytest.raises(AssertionError):
        dev.feature_match(a[:, :32], a)
    import ctypes as C
    L = wm.lib()
    idx = np.zeros(4, np.int32)
    pa, pi, host = C.c_void_p(a.ctypes.data), C.c_void_p(idx.ctypes.data), wm.WM_MEM_HOST

    def call(na=4, sa=144, nb=4, sb=144, mem=host, out=pi, out_mem=host, pb=pa):
        return L.wm_feature_match(dev._h, pa, na, sa, pb, nb, sb, mem, 0, out, None, out_mem, None)

    assert call() == wm.WM_OK
    assert call(na=0) == wm.WM_OK
    for bad in (dict(sa=128), dict(sb=128), dict(sa=134), dict(sb=146), dict(mem=5), dict(out_mem=5), dict(out=None),
                dict(na=(1 << 20) + 1), dict(nb=(1 << 20) + 1), dict(pb=None)):
        assert call(**bad) == wm.WM_ERR_ARG, bad
