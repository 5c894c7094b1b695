// The C++ drop-in away from any device: the defaults (PCL's, no test), the YAML constructor reads its six keys, a
// missing file keeps the defaults, and a ConditionalEuclideanClustering is constructed, configured and copied without
// opening a device; segment() without an input cloud returns no clusters.
#include <climits>
#include <cstdio>

#include "wave/matching/conditional_clustering.hpp"

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
    wave::ConditionalClusteringParams d{};
    CHECK(d.tolerance == 0 && d.min_cluster_size == 1 && d.max_cluster_size == INT_MAX);
    CHECK(d.max_normal_angle < 0 && d.max_scalar_diff < 0 && d.normal_k == 0);
    wave::ConditionalClusteringParams y{std::string(argv[1])};
    CHECK(y.tolerance == 0.5 && y.min_cluster_size == 10 && y.max_cluster_size == 25000);
    CHECK(y.max_normal_angle == 0.5235988 && y.max_scalar_diff == -1 && y.normal_k == 10);
    wave::ConditionalClusteringParams missing{std::string("/nonexistent/conditional.yaml")};  // logs, keeps the defaults
    CHECK(missing.tolerance == 0 && missing.max_normal_angle < 0 && missing.normal_k == 0);
    wave::ConditionalEuclideanClustering<pcl::PointXYZ> plain;
    CHECK(plain.getClusterTolerance() == 0 && plain.getMinClusterSize() == 1 && plain.getMaxClusterSize() == INT_MAX);
    CHECK(!plain.hasNormalTest() && !plain.hasScalarTest() && plain.getNormalKSearch() == 0);
    wave::ConditionalEuclideanClustering<pcl::PointXYZ> cec{y};
    CHECK(cec.getClusterTolerance() == 0.5 && cec.getMinClusterSize() == 10 && cec.getMaxClusterSize() == 25000);
    CHECK(cec.hasNormalTest() && !cec.hasScalarTest() && cec.getMaxNormalAngle() == 0.5235988 && cec.getNormalKSearch() == 10);
    cec.setClusterTolerance(0.25);
    cec.setMinClusterSize(3);
    cec.setMaxClusterSize(77);
    cec.setMaxScalarDifference(0.125);
    cec.setNormalKSearch(12);
    auto copy = cec;
    CHECK(copy.getClusterTolerance() == 0.25 && copy.getMinClusterSize() == 3 && copy.getMaxClusterSize() == 77);
    CHECK(copy.hasNormalTest() && copy.hasScalarTest() && copy.getMaxScalarDifference() == 0.125 && copy.getNormalKSearch() == 12);
    plain = cec;
    CHECK(plain.getClusterTolerance() == 0.25 && plain.getMaxClusterSize() == 77 && plain.hasScalarTest());
    plain.clearConditions();
    CHECK(!plain.hasNormalTest() && !plain.hasScalarTest() && cec.hasNormalTest());
    CHECK(!plain.getInputCloud());
    std::vector<pcl::PointIndices> clusters(2);
    plain.segment(clusters);  // no input cloud: nothing, and no device
    CHECK(clusters.empty());
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
