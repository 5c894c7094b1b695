"""wm_corr_ransac and wave::CorrespondenceRejectorSampleConsensus<PointT> without a device: the symbols are exported and
declared, the structures have the header's layout and PCL's defaults, every argument error is found before a device is
touched, fewer than three correspondences (and, in host memory, fewer than three VALID ones) have no model without a
device, the headers compile on their own, and the class is constructed, copied and runs its no-model path with no
device visible."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libwave_amd")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_symbols_structures_and_defaults(wm):
    for name in ("wm_corr_ransac", "wm_corr_ransac_default_params", "wm_corr_hypothesis", "wm_debug_corr_hypotheses"):
        assert name in wm.declared_symbols() and hasattr(wm.lib(), name)
    assert (wm.WM_CORR_NONE, wm.WM_CORR_INLIER, wm.WM_CORR_OUTLIER) == (0, 1, 2)
    assert C.sizeof(wm.CorrRansacParams) == 48 and C.sizeof(wm.CorrRansacStats) == 112
    assert wm.CorrRansacStats.model.offset == 60 and wm.CorrRansacStats.kernel_ms.offset == 108
    p = wm.corr_ransac_params()
    assert (p.inlier_threshold, p.max_iterations, p.probability, p.refine_model, p.min_sample_distance, p.seed) == \
        (0.05, 1000, 0.99, 0, -1.0, 0)
    p = wm.corr_ransac_params(dict(max_iterations=7), refine_model=1, seed=2 ** 63 + 5)
    assert p.max_iterations == 7 and p.refine_model == 1 and p.seed == 2 ** 63 + 5
    with pytest.raises(AttributeError):
        wm.corr_ransac_params(distance_threshold=1.0)


def test_the_option_is_in_the_table():
    src = open(os.path.join(LIB, "csrc", "wm_ctx.hip")).read()
    assert '{"corr_round", "WM_TUNE_CORR_ROUND", &wm_ctx::tune_corr_round, nullptr, 1, 1024, 0}' in src


def call(wm, ctx=C.c_void_p(1), n_src=10, n_tgt=10, m=10, stride=12, mem=None, out_mem=None, params="p", T="T", n_out="n_out",
         cap=10, idx="idx", src="src", tgt="tgt", match="match", query=None, **fields):
    """The entry point with one bad argument; `ctx` defaults to a pointer that must never be followed."""
    a = np.zeros((10, 4), np.float32)
    b = np.zeros((10, 4), np.float32)
    mi = np.zeros(16, np.int32)
    qi = np.zeros(16, np.int32)
    out = np.zeros(16, np.int32)
    k = C.c_size_t(77)
    Tm = np.full(16, 5.0)
    p = wm.corr_ransac_params(fields)
    rc = wm.lib().wm_corr_ransac(
        ctx, C.c_void_p(a.ctypes.data) if src == "src" else None, n_src, C.c_void_p(b.ctypes.data) if tgt == "tgt" else None,
        n_tgt, stride, C.c_void_p(qi.ctypes.data) if query == "query" else None,
        C.c_void_p(mi.ctypes.data) if match == "match" else None, m, wm.WM_MEM_HOST if mem is None else mem,
        C.byref(p) if params == "p" else None, Tm.ctypes.data_as(C.POINTER(C.c_double)) if T == "T" else None,
        C.c_void_p(out.ctypes.data) if idx == "idx" else None, cap, wm.WM_MEM_HOST if out_mem is None else out_mem,
        C.byref(k) if n_out == "n_out" else None, None, None)
    assert np.all(Tm == 5.0)  # T_out is written only with a model
    return rc, k.value


@pytest.mark.parametrize("bad", [
    dict(ctx=None), dict(params=None), dict(T=None), dict(n_out=None), dict(src=None), dict(tgt=None), dict(match=None),
    dict(idx=None), dict(stride=8), dict(stride=10), dict(stride=14), dict(mem=5), dict(out_mem=7),
    dict(n_src=0x7FFFFFF1), dict(n_tgt=0x7FFFFFF1), dict(m=(1 << 20) + 1, query="query"), dict(m=11), dict(m=16, n_src=15),
    dict(inlier_threshold=0.0), dict(inlier_threshold=-1.0), dict(inlier_threshold=float("nan")),
    dict(inlier_threshold=float("inf")),
    dict(max_iterations=0), dict(max_iterations=-5),
    dict(probability=0.0), dict(probability=1.0), dict(probability=-0.5), dict(probability=float("nan")),
    dict(min_sample_distance=float("nan")), dict(min_sample_distance=float("inf")),
], ids=lambda b: "-".join("%s=%s" % kv for kv in sorted(b.items()))[:60])
def test_argument_errors_without_a_device(wm, bad):
    rc, k = call(wm, **bad)
    assert rc == wm.WM_ERR_ARG
    assert k == 77  # nothing is written


@pytest.mark.parametrize("m", [0, 1, 2])
def test_fewer_than_three_entries_have_no_model_without_a_device(wm, m):
    rc, k = call(wm, m=m)
    assert rc == wm.WM_NOT_CONVERGED and k == 0
    rc, k = call(wm, m=m, match=None if m == 0 else "match", cap=0, idx=None, mem=wm.WM_MEM_DEVICE, out_mem=wm.WM_MEM_DEVICE)
    assert rc == wm.WM_NOT_CONVERGED and k == 0


def test_no_valid_entry_has_no_model_without_a_device(wm):
    L = wm.lib()
    src = np.arange(30, dtype=np.float32).reshape(10, 3)
    tgt = src + np.float32(1)
    st = wm.CorrRansacStats()
    st.iterations = 9
    p = wm.corr_ransac_params()
    T = np.full(16, 5.0)
    out = np.zeros(16, np.int32)

    def run(mi, qi=None, n_src=10, n_tgt=10, a=src, b=tgt):
        k = C.c_size_t(5)
        rc = L.wm_corr_ransac(C.c_void_p(1), C.c_void_p(a.ctypes.data), n_src, C.c_void_p(b.ctypes.data), n_tgt, 12,
                              C.c_void_p(qi.ctypes.data) if qi is not None else None, C.c_void_p(mi.ctypes.data), len(mi),
                              wm.WM_MEM_HOST, C.byref(p), T.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(out.ctypes.data),
                              16, wm.WM_MEM_HOST, C.byref(k), None, C.byref(st))
        assert rc == wm.WM_NOT_CONVERGED and k.value == 0 and np.all(T == 5.0)
        assert (st.iterations, st.skipped, st.rounds, st.hypotheses, st.best_hypothesis, st.n_valid) == (0, 0, 0, 0, -1, 0)

    run(np.full(10, -1, np.int32))                                   # feature_match's "no match" everywhere
    run(np.array([0, 1, -1, 10, 11, -3, 99, -1, -1, -1], np.int32))  # two valid entries
    run(np.arange(10, dtype=np.int32), np.array([0, 1, -1, 10, 11, -3, 99, -1, -1, 2 ** 31 - 1], np.int32))
    run(np.arange(10, dtype=np.int32), n_tgt=0)                      # an empty cloud on either side
    run(np.zeros(0, np.int32), n_src=0)
    bad = src.copy()
    bad[2:, 1] = np.nan                                              # two finite source points
    run(np.arange(10, dtype=np.int32), a=bad)
    bad = tgt.copy()
    bad[:8, 2] = np.inf
    run(np.arange(10, dtype=np.int32), b=bad)


def test_the_host_rule_needs_no_device(wm):
    p = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32)
    q = np.array([[1, 2, 3], [1, 6, 3], [-2, 2, 3]], np.float32)  # a quarter turn about z, then (1, 2, 3)
    flag, T = wm.corr_hypothesis(p, q, 0.0)
    assert flag == 1
    want = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float64)
    assert np.abs(T - want).max() <= 4 * 2.0 ** -23
    flag, T = wm.corr_hypothesis(p, q, 9.0)  # |p2 - p0|^2 = 9 is not > 9
    assert flag == 0 and not T.any()
    assert wm.lib().wm_corr_hypothesis(None, None, C.c_float(0), None) == wm.WM_ERR_ARG


@needs_gxx
@pytest.mark.parametrize("header", ["wave/matching/correspondence_rejection.hpp",
                                    "wave/matching/impl/correspondence_rejection.hpp"])
def test_headers_compile_standalone(tmp_path, header):
    src = tmp_path / "one.cpp"
    src.write_text("#include <%s>\n" % header)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_the_rule_header_compiles_with_a_plain_compiler(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text('#include "wm_corr_rule.hpp"\nint main() { float T[12]; const float p[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};\n'
                   "return wm::corr_hypothesis(p, p, 0.f, T) == wm::kCorrValid ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-ffp-contract=off", "-I" + os.path.join(LIB, "csrc"), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@needs_gxx
def test_construction_copies_and_the_no_model_path_without_a_device(tmp_path):
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "corr_cpu.cpp"
    src.write_text("""
#include <cstdio>
#include "wave/matching/correspondence_rejection.hpp"
static bool identity(const Eigen::Matrix4d &m) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (m(r, c) != (r == c ? 1.0 : 0.0)) return false;
    return true;
}
int main(int argc, char **argv) {
    using Cloud = pcl::PointCloud<pcl::PointXYZ>;
    wave::CorrespondenceRejectorSampleConsensus<pcl::PointXYZ> a;
    a.setInlierThreshold(0.25);
    a.setMaximumIterations(17);
    a.setRefineModel(true);
    a.setSeed(3);
    a.setMinSampleDistance(0.5);
    a.setProbability(0.9);
    wave::CorrespondenceRejectorSampleConsensus<pcl::PointXYZ> b = a, c;
    c = b;
    bool ok = c.getInlierThreshold() == 0.25 && c.getMaximumIterations() == 17 && c.getRefineModel() && !c.getInputSource() &&
              identity(c.getBestTransformation());
    // no clouds: the input and the identity (a LOG_ERROR), no device
    std::vector<pcl::Correspondence> in(5), out(1);
    for (int e = 0; e < 5; ++e) in[e] = pcl::Correspondence(e, e, 0.5f * e);
    c.getRemainingCorrespondences(in, out);
    ok = ok && out.size() == 5 && out[4].index_match == 4 && identity(c.getBestTransformation());
    // clouds, but two correspondences / no valid one: no model, no device
    auto cloud = boost::make_shared<Cloud>();
    for (int i = 0; i < 8; ++i) {
        pcl::PointXYZ p;
        p.x = (float) i, p.y = (float) (i * i), p.z = 1.f;
        cloud->push_back(p);
    }
    c.setInputSource(cloud);
    c.setInputTarget(cloud);
    std::vector<pcl::Correspondence> two(in.begin(), in.begin() + 2);
    c.getRemainingCorrespondences(two, out);
    ok = ok && out.size() == 2 && identity(c.getBestTransformation());
    for (auto &e : in) e.index_match = 99;
    c.getRemainingCorrespondences(in, out);
    ok = ok && out.size() == 5 && out[0].index_match == 99 && identity(c.getBestTransformation());
    out.clear();
    c.getRemainingCorrespondences(out, out);  // nothing in, nothing out
    ok = ok && out.empty();
    wave::CorrespondenceRejectionParams missing("/nonexistent/correspondence_rejection.yaml");  // logs, keeps the defaults
    ok = ok && missing.inlier_threshold == 0.05 && missing.max_iterations == 1000 && missing.refine_model == 0 &&
         missing.min_sample_distance == -1.0 && missing.probability == 0.99;
    if (argc > 1) {
        wave::CorrespondenceRejectionParams file(argv[1]);
        ok = ok && file.inlier_threshold == 0.1 && file.max_iterations == 400 && file.refine_model == 1;
    }
    std::printf("failed checks: %d\\n", ok ? 0 : 1);
    return ok ? 0 : 1;
}
""")
    exe = str(tmp_path / "corr_cpu")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                        exe, "-L" + LIB, "-lwave_matching", "-lwavematch_hip", "-Wl,-rpath," + LIB, "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "config", "correspondence_rejection.yaml")],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "failed checks: 0" in r.stdout, r.stdout + r.stderr[-1000:]
