// The C++ drop-in away from any device: the defaults are PCL's, the YAML constructor reads its three keys, a missing
// file keeps the defaults, and a EuclideanClusterExtraction is constructed, configured and copied without opening a
// device; extract() without an input cloud returns no clusters.
#include <climits>
#include <cstdio>

#include "wave/matching/cluster_extraction.hpp"

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    wave::ClusterExtractionParams d{};
    CHECK(d.tolerance == 0 && d.min_cluster_size == 1 && d.max_cluster_size == INT_MAX);
    wave::ClusterExtractionParams y{std::string(argv[1])};
    CHECK(y.tolerance == 0.5 && y.min_cluster_size == 10 && y.max_cluster_size == 25000);
    wave::ClusterExtractionParams missing{std::string("/nonexistent/cluster.yaml")};  // logs, keeps the defaults
    CHECK(missing.tolerance == 0 && missing.min_cluster_size == 1 && missing.max_cluster_size == INT_MAX);
    wave::EuclideanClusterExtraction<pcl::PointXYZ> plain;
    CHECK(plain.getClusterTolerance() == 0 && plain.getMinClusterSize() == 1 && plain.getMaxClusterSize() == INT_MAX);
    wave::EuclideanClusterExtraction<pcl::PointXYZ> ec{y};
    CHECK(ec.getClusterTolerance() == 0.5 && ec.getMinClusterSize() == 10 && ec.getMaxClusterSize() == 25000);
    ec.setClusterTolerance(0.25);
    ec.setMinClusterSize(3);
    ec.setMaxClusterSize(77);
    auto copy = ec;
    CHECK(copy.getClusterTolerance() == 0.25 && copy.getMinClusterSize() == 3 && copy.getMaxClusterSize() == 77);
    plain = ec;
    CHECK(plain.getClusterTolerance() == 0.25 && plain.getMaxClusterSize() == 77);
    CHECK(!plain.getInputCloud());
    std::vector<pcl::PointIndices> clusters(2);
    plain.extract(clusters);  // no input cloud: nothing, and no device
    CHECK(clusters.empty());
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
