// wave::EuclideanClusterExtraction<pcl::PointXYZ> on a scan: YAML params, extract() against the clusters the C ABI
// (wm_cluster_extract, called here on a context of its own) gives for the same cloud and parameters; setters and
// getters; a copy works on a context of its own; a 32-byte point type through the impl header; bad parameters give
// no clusters.
#include <cstdio>
#include <string>
#include <vector>

#include "wave/matching/cluster_extraction.hpp"
#include "wave/matching/impl/cluster_extraction.hpp"
#include "wavematch.h"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::EuclideanClusterExtraction<Point32>;

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

static Clusters viaAbi(wm_ctx *ctx, const Cloud &in, double tolerance, int min_size, int max_size) {
    wm_cluster_params p;
    wm_cluster_default_params(&p);
    p.tolerance = tolerance, p.min_cluster_size = min_size, p.max_cluster_size = max_size;
    std::vector<int32_t> idx(in.size());
    std::vector<uint32_t> off(in.size() + 1);
    size_t k = 0, m = 0;
    const int rc = wm_cluster_extract(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST, &p, nullptr,
                                      idx.data(), idx.size(), off.data(), in.size(), WM_MEM_HOST, &k, &m, nullptr);
    CHECK(rc == WM_OK);
    Clusters out(rc == WM_OK ? k : 0);
    for (size_t c = 0; c < out.size(); ++c) out[c].indices.assign(idx.begin() + off[c], idx.begin() + off[c + 1]);
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

    wave::ClusterExtractionParams params{config};
    CHECK(params.tolerance == 0.5 && params.min_cluster_size == 10 && params.max_cluster_size == 25000);
    wave::EuclideanClusterExtraction<pcl::PointXYZ> ec{params};
    ec.setInputCloud(input);
    CHECK(ec.getInputCloud() == input);
    Clusters got;
    ec.extract(got);
    const Clusters want = viaAbi(ctx, *input, 0.5, 10, 25000);
    CHECK(same(got, want));
    CHECK(got.size() > 1);
    size_t total = 0;
    for (size_t c = 0; c < got.size(); ++c) {
        CHECK(got[c].indices.size() >= 10 && got[c].indices.size() <= 25000);
        if (c) CHECK(got[c].indices.size() <= got[c - 1].indices.size());
        for (size_t j = 1; j < got[c].indices.size(); ++j) CHECK(got[c].indices[j] > got[c].indices[j - 1]);
        total += got[c].indices.size();
    }
    CHECK(total <= input->size());
    std::printf("tolerance 0.5, sizes 10 ... 25000: %zu clusters, %zu of %zu points, the largest %zu\n", got.size(), total,
                input->size(), got.empty() ? (size_t) 0 : got[0].indices.size());
    Clusters again;  // a second call extracts afresh
    ec.extract(again);
    CHECK(same(again, want));

    // setters and getters; a copy has its own context and the same settings
    ec.setClusterTolerance(0.3);
    ec.setMinClusterSize(2);
    ec.setMaxClusterSize(500);
    CHECK(ec.getClusterTolerance() == 0.3 && ec.getMinClusterSize() == 2 && ec.getMaxClusterSize() == 500);
    auto copy = ec;
    Clusters a, b;
    copy.extract(a);
    ec.extract(b);
    const Clusters want2 = viaAbi(ctx, *input, 0.3, 2, 500);
    CHECK(same(a, want2) && same(b, want2) && !same(a, want));
    std::printf("tolerance 0.3, sizes 2 ... 500: %zu clusters\n", a.size());

    // a 32-byte point type (stride 32): the same clusters
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &p : input->points) in32->push_back(Point32{p.x, p.y, p.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::EuclideanClusterExtraction<Point32> e32{params};
    e32.setInputCloud(in32);
    Clusters c32;
    e32.extract(c32);
    CHECK(same(c32, want));

    // bad parameters: LOG_ERROR and no clusters
    wave::EuclideanClusterExtraction<pcl::PointXYZ> bad;  // PCL's default tolerance 0
    bad.setInputCloud(input);
    Clusters none(3);
    bad.extract(none);
    CHECK(none.empty());
    // max < min is legal and keeps nothing
    ec.setMinClusterSize(50);
    ec.setMaxClusterSize(5);
    ec.extract(none);
    CHECK(none.empty());

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
