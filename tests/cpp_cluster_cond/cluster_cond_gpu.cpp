// wave::ConditionalEuclideanClustering<pcl::PointXYZ> on a scan: YAML params, segment() against the clusters the C ABI
// (wm_estimate_normals + wm_cluster_extract_cond, called here on a context of its own) gives for the same cloud and
// parameters; setNormalKSearch against the C ABI fed with wm_estimate_normals' output; setInputAttributes with a 32-byte
// stride; clearConditions() against EuclideanClusterExtraction::extract; a copy works on a context of its own; the
// error paths give no clusters.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "wave/matching/cluster_extraction.hpp"
#include "wave/matching/conditional_clustering.hpp"
#include "wavematch.h"

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

using Cloud = pcl::PointCloud<pcl::PointXYZ>;
using Clusters = std::vector<pcl::PointIndices>;

static std::vector<float> normalsViaAbi(wm_ctx *ctx, const Cloud &in, int k) {
    std::vector<float> nrm(4 * in.size());
    CHECK(wm_set_source(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST) == WM_OK);
    CHECK(wm_set_target(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST) == WM_OK);
    CHECK(wm_estimate_normals(ctx, 1, k, nrm.data(), WM_MEM_HOST) == WM_OK);
    return nrm;
}

static Clusters viaAbi(wm_ctx *ctx, const Cloud &in, const float *attr, size_t attr_stride, double tolerance, int min_size,
                       int max_size, int flags, double angle, double diff) {
    wm_cluster_params p;
    wm_cluster_default_params(&p);
    p.tolerance = tolerance, p.min_cluster_size = min_size, p.max_cluster_size = max_size;
    wm_cluster_cond c;
    wm_cluster_cond_default(&c);
    c.flags = flags, c.max_normal_angle = angle, c.max_scalar_diff = diff;
    std::vector<int32_t> idx(in.size());
    std::vector<uint32_t> off(in.size() + 1);
    size_t k = 0, m = 0;
    const int rc = wm_cluster_extract_cond(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST, attr,
                                           attr_stride, WM_MEM_HOST, &p, &c, nullptr, idx.data(), idx.size(), off.data(),
                                           in.size(), WM_MEM_HOST, &k, &m, nullptr);
    CHECK(rc == WM_OK);
    Clusters out(rc == WM_OK ? k : 0);
    for (size_t j = 0; j < out.size(); ++j) out[j].indices.assign(idx.begin() + off[j], idx.begin() + off[j + 1]);
    return out;
}

static bool same(const Clusters &a, const Clusters &b) {
    if (a.size() != b.size()) return false;
    for (size_t c = 0; c < a.size(); ++c)
        if (a[c].indices != b[c].indices) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    auto input = boost::make_shared<Cloud>();
    if (pcl::io::loadPCDFile(scan, *input) != 0) return 3;
    wm_ctx *ctx = nullptr;
    if (wm_ctx_create(&ctx, 0) != WM_OK) return 4;

    // the YAML fixture: the normal test at 30 degrees on normals from 10 neighbours, no scalar test
    wave::ConditionalClusteringParams params{config};
    CHECK(params.tolerance == 0.5 && params.min_cluster_size == 10 && params.max_cluster_size == 25000);
    CHECK(params.max_normal_angle == 0.5235988 && params.max_scalar_diff == -1 && params.normal_k == 10);
    wave::ConditionalEuclideanClustering<pcl::PointXYZ> cec{params};
    CHECK(cec.hasNormalTest() && !cec.hasScalarTest() && cec.getNormalKSearch() == 10);
    cec.setInputCloud(input);
    CHECK(cec.getInputCloud() == input);
    Clusters got;
    cec.segment(got);
    const std::vector<float> nrm = normalsViaAbi(ctx, *input, 10);
    const Clusters want = viaAbi(ctx, *input, nrm.data(), 16, 0.5, 10, 25000, WM_CLUSTER_COND_NORMAL, 0.5235988, 0.0);
    CHECK(same(got, want));
    CHECK(got.size() > 1);
    size_t total = 0;
    for (size_t c = 0; c < got.size(); ++c) {
        CHECK(got[c].indices.size() >= 10 && got[c].indices.size() <= 25000);
        if (c) CHECK(got[c].indices.size() <= got[c - 1].indices.size());
        for (size_t j = 1; j < got[c].indices.size(); ++j) CHECK(got[c].indices[j] > got[c].indices[j - 1]);
        total += got[c].indices.size();
    }
    std::printf("tolerance 0.5, normals within 30 degrees (k = 10): %zu clusters, %zu of %zu points, the largest %zu\n",
                got.size(), total, input->size(), got.empty() ? (size_t) 0 : got[0].indices.size());
    Clusters again;  // a second call segments afresh
    cec.segment(again);
    CHECK(same(again, want));

    // clearConditions(): EuclideanClusterExtraction::extract's clusters, and other clusters than with the test
    wave::EuclideanClusterExtraction<pcl::PointXYZ> ec;
    ec.setClusterTolerance(0.5);
    ec.setMinClusterSize(10);
    ec.setMaxClusterSize(25000);
    ec.setInputCloud(input);
    Clusters plain, cleared;
    ec.extract(plain);
    auto none_on = cec;
    none_on.clearConditions();
    CHECK(!none_on.hasNormalTest() && !none_on.hasScalarTest());
    none_on.segment(cleared);
    CHECK(same(cleared, plain) && !plain.empty() && !same(plain, want));

    // setInputAttributes with a 32-byte stride (the normals' records with a payload behind); both tests; a copy has
    // its own context and the same settings
    std::vector<float> wide(8 * input->size(), NAN);
    for (size_t i = 0; i < input->size(); ++i)
        for (int j = 0; j < 4; ++j) wide[8 * i + j] = nrm[4 * i + j];
    wave::ConditionalEuclideanClustering<pcl::PointXYZ> own;
    own.setClusterTolerance(0.3);
    own.setMinClusterSize(2);
    own.setMaxClusterSize(500);
    own.setMaxNormalAngle(0.3);
    own.setMaxScalarDifference(0.02);
    own.setInputAttributes(wide.data(), input->size(), 32);
    own.setInputCloud(input);
    CHECK(own.getClusterTolerance() == 0.3 && own.getMinClusterSize() == 2 && own.getMaxClusterSize() == 500);
    CHECK(own.getMaxNormalAngle() == 0.3 && own.getMaxScalarDifference() == 0.02 && own.hasNormalTest() && own.hasScalarTest());
    auto copy = own;
    Clusters a, b;
    copy.segment(a);
    own.segment(b);
    const Clusters want2 = viaAbi(ctx, *input, nrm.data(), 16, 0.3, 2, 500, WM_CLUSTER_COND_NORMAL | WM_CLUSTER_COND_SCALAR, 0.3, 0.02);
    CHECK(same(a, want2) && same(b, want2) && !a.empty() && !same(a, want));
    std::printf("tolerance 0.3, sizes 2 ... 500, normals within 0.3 rad, curvatures within 0.02: %zu clusters\n", a.size());
    own.setNormalKSearch(10);  // takes precedence over the array: the same normals, estimated by the class
    own.segment(b);
    CHECK(same(b, want2));
    own.setNormalKSearch(0);

    // the error paths: LOG_ERROR and no clusters
    Clusters none(3);
    wave::ConditionalEuclideanClustering<pcl::PointXYZ> bad;  // PCL's default tolerance 0
    bad.setInputCloud(input);
    bad.segment(none);
    CHECK(none.empty());
    none.resize(3);
    own.setInputAttributes(nullptr, 0);  // a test without attributes
    own.segment(none);
    CHECK(none.empty());
    none.resize(3);
    own.setInputAttributes(wide.data(), input->size() - 1, 32);  // a record short
    own.segment(none);
    CHECK(none.empty());
    none.resize(3);
    own.setInputAttributes(wide.data(), input->size(), 12);  // a bad stride
    own.segment(none);
    CHECK(none.empty());
    none.resize(3);
    own.setInputAttributes(wide.data(), input->size(), 32);
    own.setMaxNormalAngle(2.0);  // beyond pi / 2
    own.segment(none);
    CHECK(none.empty());
    none.resize(3);
    own.setMaxNormalAngle(0.3);
    own.setMaxScalarDifference(-0.5);
    own.segment(none);
    CHECK(none.empty());
    none.resize(3);
    own.setMaxScalarDifference(0.02);
    own.setNormalKSearch(40);  // more neighbours than the search keeps
    own.segment(none);
    CHECK(none.empty());
    auto few = boost::make_shared<Cloud>();  // fewer finite points than neighbours
    for (int i = 0; i < 5; ++i) few->push_back(pcl::PointXYZ(0.1f * i, 0.f, 0.f));
    none.resize(3);
    own.setNormalKSearch(10);
    own.setInputCloud(few);
    own.segment(none);
    CHECK(none.empty());
    own.clearConditions();  // without a test the five points need no attributes: one cluster
    own.segment(none);
    CHECK(none.size() == 1 && none[0].indices.size() == 5);

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
