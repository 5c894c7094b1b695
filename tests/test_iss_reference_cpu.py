"""wm_iss_keypoints without a device.

  a. the checker's two forms (tests/iss_reference.py: every pair with Python integers / a kd-tree's candidates with
     int64 sums) against each other on every case tests/test_iss_gpu.py compares the device on.
  b. the rule against PCL's own arithmetic (iss_reference.pcl_literal: double sums in list order, eigvalsh, PCL's
     tests) on the six base cases: the same salient set and the same keypoint set, a point left out only when a
     decision of its own lies within 1e-6 relative of its bound, at most 1 % of the finite points.
  c. the by-hand cases.
  d. the bindings, the structures, every argument error and the empty call, which come before a device is touched;
     wm_iss_third against the checker, bit for bit; wm_gather_records in host memory."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

import iss_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BASE = ["scene-1.0", "scene-6x", "rings-1.0", "rings-6x", "scan-1.0", "scan-6x"]


def same(a, b):
    for k in ("indices", "labels", "counts", "sums"):
        assert np.array_equal(a[k], b[k]), k
    assert a["third"].tobytes() == b["third"].tobytes()
    assert (a["n_finite"], a["n_salient"], a["n_keypoints"]) == (b["n_finite"], b["n_salient"], b["n_keypoints"])


# ---- a. the two forms

def test_the_base_cases_are_the_six():
    assert sorted(IR.base_cases()) == sorted(BASE)


@pytest.mark.parametrize("name", BASE)
def test_the_two_forms_agree_on_the_base_cases(name):
    c, rs, rn = IR.base_cases()[name]
    ref = IR.reference(name)
    same(IR.keypoints_brute(c, rs, rn), ref)
    print(name, "salient", ref["n_salient"], "keypoints", ref["n_keypoints"])
    assert 10 <= ref["n_keypoints"] <= 400 and ref["n_salient"] > ref["n_keypoints"]


def test_the_two_forms_agree_on_the_large_scene():
    """synth.scene(20000, 42) at (1.86, 1.24): both forms, and PCL's own arithmetic (pcl_literal, with no point left
    out), give 15 503 salient points and 654 keypoints."""
    cloud, ref = IR.big_case()
    same(IR.keypoints_brute(cloud, *IR.BIG_RADII), ref)
    assert (ref["n_salient"], ref["n_keypoints"]) == (15503, 654)
    assert IR.compare_with_literal(ref, IR.pcl_literal(cloud, *IR.BIG_RADII)) == (0, 0)


variants = IR.variants


@pytest.mark.parametrize("name", sorted(variants()))
def test_the_two_forms_agree_on_the_variants(name):
    c, rs, rn, kw = variants()[name]
    same(IR.keypoints_brute(c, rs, rn, **kw), IR.keypoints(c, rs, rn, **kw))


# ---- b. PCL as it is written

@pytest.mark.parametrize("name", BASE)
def test_the_rule_gives_pcls_sets(name):
    c, rs, rn = IR.base_cases()[name]
    ref = IR.reference(name)
    lit = IR.pcl_literal(c, rs, rn)
    differ, left_out = IR.compare_with_literal(ref, lit)
    print(name, "differences", differ, "left out", left_out, "of", ref["n_finite"])
    assert differ == 0
    assert left_out <= 0.01 * ref["n_finite"]
    # the integer sums are the double sums to their quantum 2^(x - 36): an entry of the matrix is off by at most n_s half
    # quanta, the matrix by 3 n_s 2^(x - 37) in the Frobenius norm, and an eigenvalue moves by no more than that (Weyl);
    # the two eigen-solvers add a few ulps of the largest eigenvalue
    both = (ref["third"][lit["cand"]] > 0) & lit["salient"]
    bound = 3.0 * lit["n_s"] * math.ldexp(1.0, ref["x"] - 37) + 1e-12 * lit["e"][:, 2]
    assert np.all(np.abs(ref["third"][lit["cand"]] - lit["third"])[both] <= bound[both])


# ---- c. by hand

def test_a_pair_at_exactly_r2_is_out_and_one_ulp_below_is_in():
    r = 0.5
    r2 = IR.r2_of(r)
    assert float(r2) == 0.25
    at = np.array([[0, 0, 0], [0.5, 0, 0]], F)                      # d2 == r2 exactly
    below = np.array([[0, 0, 0], [np.nextafter(F(0.5), F(0)), 0, 0]], F)
    for form in (IR.keypoints, IR.keypoints_brute):
        assert list(form(at, r, r, min_neighbors=0)["counts"]) == [1, 1]
        assert list(form(below, r, r, min_neighbors=0)["counts"]) == [2, 2]


def test_an_exact_planar_lattice_has_nothing_salient():
    ref = IR.keypoints(IR.lattice(), 0.8, 0.5)
    assert ref["counts"].max() > 20 and ref["n_salient"] == 0 and ref["n_keypoints"] == 0
    assert not ref["sums"][:, [2, 4, 5]].any()  # every z product is zero


def test_a_cloud_and_its_duplicate_keep_every_keypoint_twice():
    c, rs, rn, _ = variants()["duplicate"]
    n = len(c) // 2
    ref = IR.keypoints(c, rs, rn)
    k = ref["indices"]
    assert len(k) > 4 and np.array_equal(k[:len(k) // 2] + n, k[len(k) // 2:])
    assert ref["third"][:n].tobytes() == ref["third"][n:].tobytes()


def test_gamma_zero_and_a_high_min_neighbors_give_none():
    for name in ("gamma-0", "min-neighbors-high"):
        c, rs, rn, kw = variants()[name]
        ref = IR.keypoints(c, rs, rn, **kw)
        assert ref["n_salient"] == 0 and ref["n_keypoints"] == 0 and ref["n_finite"] == len(c)


def test_every_salient_point_is_a_keypoint_below_the_spacing():
    c, rs, rn, kw = variants()["all-salient-kept"]
    ref = IR.keypoints(c, rs, rn, **kw)
    assert ref["n_salient"] > 100 and ref["n_keypoints"] == ref["n_salient"]


def test_the_restated_jacobi_finds_the_eigenvalues():
    rng = np.random.default_rng(2)
    for _ in range(50):
        m = rng.normal(size=(3, 3))
        a = m @ m.T
        got = sorted(IR.jacobi3(a.ravel()))
        assert np.allclose(got, np.linalg.eigvalsh(a), rtol=1e-12, atol=1e-14)


# ---- d. the library without a device

def test_symbols_structures_and_defaults(wm):
    for name in ("wm_iss_keypoints", "wm_iss_default_params", "wm_iss_third", "wm_gather_records"):
        assert name in wm.declared_symbols() and hasattr(wm.lib(), name)
    assert (wm.WM_ISS_NONE, wm.WM_ISS_PLAIN, wm.WM_ISS_SALIENT, wm.WM_ISS_KEYPOINT) == (0, 1, 2, 3)
    assert (IR.NONE, IR.PLAIN, IR.SALIENT, IR.KEYPOINT) == (0, 1, 2, 3)
    assert C.sizeof(wm.IssParams) == 40 and C.sizeof(wm.IssStats) == 32
    assert wm.IssParams.min_neighbors.offset == 32 and wm.IssStats.kernel_ms.offset == 24
    assert wm.WM_ISS_MAX_POINTS == 1 << 26
    header = open(os.path.join(ROOT, "include", "wavematch.h")).read()
    assert "#define WM_ISS_MAX_POINTS 0x4000000ull" in header and "#define WM_GATHER_MAX_STRIDE 65536u" in header
    p = wm.iss_params()
    assert (p.salient_radius, p.non_max_radius, p.gamma_21, p.gamma_32, p.min_neighbors) == (0.0, 0.0, 0.975, 0.975, 5)
    p = wm.iss_params(dict(salient_radius=2.0), min_neighbors=7)
    assert p.salient_radius == 2.0 and p.min_neighbors == 7
    with pytest.raises(AttributeError):
        wm.iss_params(border_radius=1.0)


def test_the_option_is_in_the_table():
    src = open(os.path.join(ROOT, "libwave_amd", "csrc", "wm_ctx.hip")).read()
    assert '{"iss_cell_div", "WM_TUNE_ISS_CELL_DIV", nullptr, &wm_ctx::tune_iss_cell_div, 0.5, 8, 0}' in src
    assert "`iss_cell_div` | `WM_TUNE_ISS_CELL_DIV` | 2 |" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def call(wm, ctx=C.c_void_p(1), n=10, stride=12, mem=None, out_mem=None, params="p", n_out="n_out", cap=10, idx="idx", pts="pts",
         **fields):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    a = np.zeros((10, 4), np.float32)
    out = np.zeros(16, np.int32)
    k = C.c_size_t(77)
    p = wm.iss_params(dict(salient_radius=1.0, non_max_radius=0.5), **fields)
    rc = wm.lib().wm_iss_keypoints(ctx, C.c_void_p(a.ctypes.data) if pts == "pts" else None, n, stride,
                                   wm.WM_MEM_HOST if mem is None else mem, C.byref(p) if params == "p" else None,
                                   C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap,
                                   wm.WM_MEM_HOST if out_mem is None else out_mem, C.byref(k) if n_out == "n_out" else None,
                                   None, None, None, None)
    return rc, k.value


@pytest.mark.parametrize("bad", [
    dict(ctx=None), dict(params=None), dict(n_out=None), dict(pts=None), dict(idx=None), dict(stride=8), dict(stride=10),
    dict(stride=14), dict(mem=5), dict(out_mem=7), dict(n=(1 << 26) + 1),
    dict(salient_radius=0.0), dict(salient_radius=-1.0), dict(salient_radius=float("nan")), dict(salient_radius=float("inf")),
    dict(salient_radius=1e-20), dict(salient_radius=1e20),
    dict(non_max_radius=0.0), dict(non_max_radius=-1.0), dict(non_max_radius=float("nan")), dict(non_max_radius=float("inf")),
    dict(non_max_radius=1e-20), dict(non_max_radius=1e20),
    dict(gamma_21=-0.1), dict(gamma_21=float("nan")), dict(gamma_21=float("inf")),
    dict(gamma_32=-0.1), dict(gamma_32=float("nan")), dict(gamma_32=float("inf")),
    dict(min_neighbors=-1),
], ids=lambda b: "-".join("%s=%s" % kv for kv in sorted(b.items()))[:60])
def test_argument_errors_without_a_device(wm, bad):
    rc, k = call(wm, **bad)
    assert rc == wm.WM_ERR_ARG
    assert k == 77  # nothing is written


def test_an_empty_cloud_is_ok_without_a_device(wm):
    assert call(wm, n=0) == (wm.WM_OK, 0)
    assert call(wm, n=0, pts=None, idx=None, cap=0, mem=wm.WM_MEM_DEVICE, out_mem=wm.WM_MEM_DEVICE) == (wm.WM_OK, 0)


def test_wm_iss_third_equals_the_checker_bit_for_bit(wm):
    ref = IR.reference("scan-1.0")
    cand = np.nonzero(ref["finite"])[0]
    x = ref["x"]
    pos = 0
    for i in range(0, len(cand), 3):
        s, n_s = ref["sums"][i], int(ref["counts"][cand[i]])
        got = wm.iss_third(s, n_s, x)
        assert struct.pack("<d", got) == struct.pack("<d", float(ref["third"][cand[i]])), (i, s)
        pos += got > 0
    assert pos > 100
    # the edges of the step
    u = 1 << 36
    assert wm.iss_third([4 * u, 0, 0, 2 * u, 0, u], 10, 0) == 1.0 == IR.third_from_sums([4 * u, 0, 0, 2 * u, 0, u], 10, 0)
    assert wm.iss_third([4 * u, 0, 0, 2 * u, 0, u], 4, 0) == 0.0
    assert wm.iss_third([4 * u, 0, 0, 2 * u, 0, u], 10, 0, gamma_21=0.5) == 0.0
    assert wm.iss_third([0] * 6, 10, 0) == 0.0 == IR.third_from_sums([0] * 6, 10, 0)
    assert wm.iss_third([-4 * u, 0, 0, -2 * u, 0, -u], 10, 0) == 0.0
    L = wm.lib()
    p = wm.iss_params()
    s = (C.c_int64 * 6)()
    out = C.c_double(5.0)
    assert L.wm_iss_third(None, 1, 0, C.byref(p), C.byref(out)) == wm.WM_ERR_ARG
    assert L.wm_iss_third(s, 1, 0, None, C.byref(out)) == wm.WM_ERR_ARG
    assert L.wm_iss_third(s, 1, 0, C.byref(p), None) == wm.WM_ERR_ARG
    assert L.wm_iss_third(s, 1, 129, C.byref(p), C.byref(out)) == wm.WM_ERR_ARG
    assert L.wm_iss_third(s, 1, -126, C.byref(p), C.byref(out)) == wm.WM_ERR_ARG
    assert out.value == 5.0
    assert math.frexp(float(IR.r2_of(1.0)))[1] == 1 and IR.exponent_of(IR.r2_of(0.5)) == -1


def gather(wm, ctx=C.c_void_p(1), n=10, stride=132, m=4, mem=None, src="src", idx="idx", dst="dst", index=(3, 0, 3, 9)):
    a = np.arange(10 * 36, dtype=np.float32).reshape(10, 36)
    i = np.array(index, np.int32)
    d = np.full((8, 36), -1.0, np.float32)
    rc = wm.lib().wm_gather_records(ctx, C.c_void_p(a.ctypes.data) if src == "src" else None, n, stride,
                                    C.c_void_p(i.ctypes.data) if idx == "idx" else None, m, C.c_void_p(d.ctypes.data) if dst == "dst" else None,
                                    wm.WM_MEM_HOST if mem is None else mem)
    return rc, a, d


def test_gather_records_in_host_memory_needs_no_device(wm):
    rc, a, d = gather(wm, stride=144)
    assert rc == wm.WM_OK and np.array_equal(d[:4], a[[3, 0, 3, 9]]) and np.all(d[4:] == -1.0)
    rc, a, d = gather(wm, stride=132)  # records of 33 floats packed one behind the other
    flat = a.ravel()
    assert rc == wm.WM_OK and np.array_equal(d.ravel()[:4 * 33], np.concatenate([flat[k * 33:(k + 1) * 33] for k in (3, 0, 3, 9)]))
    for bad in (dict(ctx=None), dict(stride=0), dict(stride=130), dict(stride=65540), dict(mem=3), dict(src=None), dict(idx=None),
                dict(dst=None), dict(n=0x7FFFFFF1), dict(m=0x7FFFFFF1), dict(index=(3, 0, 10, 9)), dict(index=(3, -1, 3, 9)),
                dict(n=0)):
        rc, a, d = gather(wm, **bad)
        assert rc == wm.WM_ERR_ARG, bad
        assert np.all(d == -1.0), bad  # nothing is written
    assert gather(wm, m=0, mem=wm.WM_MEM_DEVICE, idx=None, dst=None)[0] == wm.WM_OK
