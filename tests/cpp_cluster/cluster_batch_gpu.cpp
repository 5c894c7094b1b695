// EuclideanClusterExtraction<PointT>::extractBatch on a scan cut into four sub-clouds: one batched call equals four
// extract() calls, cluster for cluster and index for index, for pcl::PointXYZ and a 32-byte point type; a copy of the
// object works on a context of its own; an empty vector and a vector with an empty cloud; a null cloud is refused.
#include <cstdio>
#include <string>
#include <vector>

#include "wave/matching/cluster_extraction.hpp"
#include "wave/matching/impl/cluster_extraction.hpp"

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

using Clusters = std::vector<pcl::PointIndices>;

static bool same(const Clusters &a, const Clusters &b) {
    if (a.size() != b.size()) return false;
    for (size_t c = 0; c < a.size(); ++c)
        if (a[c].indices != b[c].indices) return false;
    return true;
}

template <class P, class Make>
static void run(const pcl::PointCloud<pcl::PointXYZ> &scan, const wave::ClusterExtractionParams &params, Make make) {
    using Ec = wave::EuclideanClusterExtraction<P>;
    std::vector<typename Ec::PointCloudConstPtr> clouds;
    const size_t cuts[5] = {0, scan.size() / 5, scan.size() / 2, scan.size() / 2 + 777, scan.size()};
    for (int k = 0; k < 4; ++k) {
        auto part = boost::make_shared<pcl::PointCloud<P>>();
        for (size_t i = cuts[k]; i < cuts[k + 1]; ++i) part->push_back(make(scan.points[i]));
        clouds.push_back(part);
    }
    Ec ec{params};
    std::vector<Clusters> want(4), got(7);
    for (int k = 0; k < 4; ++k) {
        ec.setInputCloud(clouds[k]);
        ec.extract(want[k]);
    }
    ec.extractBatch(clouds, got);
    CHECK(got.size() == 4);
    size_t n_clusters = 0;
    for (size_t k = 0; k < got.size() && k < 4; ++k) {
        CHECK(same(got[k], want[k]));
        n_clusters += got[k].size();
    }
    CHECK(n_clusters > 4);
    CHECK(ec.getInputCloud() == clouds[3]);
    std::printf("%zu-byte points: %zu clusters in four sub-clouds\n", sizeof(P), n_clusters);

    auto copy = ec;  // a context of its own, the same settings
    std::vector<Clusters> again;
    copy.extractBatch(clouds, again);
    CHECK(again.size() == 4);
    for (size_t k = 0; k < again.size() && k < 4; ++k) CHECK(same(again[k], want[k]));

    std::vector<typename Ec::PointCloudConstPtr> nothing;
    ec.extractBatch(nothing, got);
    CHECK(got.empty());
    std::vector<typename Ec::PointCloudConstPtr> mixed{clouds[1], boost::make_shared<pcl::PointCloud<P>>(), clouds[0]};
    ec.extractBatch(mixed, got);
    CHECK(got.size() == 3);
    if (got.size() == 3) CHECK(same(got[0], want[1]) && got[1].empty() && same(got[2], want[0]));
    mixed[1] = typename Ec::PointCloudConstPtr();
    ec.extractBatch(mixed, got);  // "cloud 1 is a null pointer"
    CHECK(got.empty());
    Ec bad;  // PCL's default tolerance 0: an argument error
    bad.extractBatch(clouds, got);
    CHECK(got.empty());
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    pcl::PointCloud<pcl::PointXYZ> scan;
    if (pcl::io::loadPCDFile(std::string(argv[1]), scan) != 0) return 3;
    wave::ClusterExtractionParams params{std::string(argv[2])};
    CHECK(params.tolerance == 0.5 && params.min_cluster_size == 10);
    run<pcl::PointXYZ>(scan, params, [](const pcl::PointXYZ &p) { return p; });
    run<Point32>(scan, params, [](const pcl::PointXYZ &p) { return Point32{p.x, p.y, p.z, 1.f, 7.f, 3.f, -1.f, 2.f}; });
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
