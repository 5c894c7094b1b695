// extractBatch links for pcl::PointXYZ (precompiled in libwave_matching.so) and for a 32-byte point type (through the
// impl header).  No device here: an empty queue returns before one is needed, a null cloud is refused before one is
// opened, and a queue that needs one logs the failure and gives nothing.
#include <cstdio>
#include <vector>

#include "wave/matching/cluster_extraction.hpp"
#include "wave/matching/impl/cluster_extraction.hpp"

struct alignas(16) Point32 {
    float x, y, z, pad;
    float intensity, ring;
    int index, scan;
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

template <class P>
static void none() {
    using Ec = wave::EuclideanClusterExtraction<P>;
    Ec ec;
    ec.setClusterTolerance(0.5);
    std::vector<typename Ec::PointCloudConstPtr> clouds;
    std::vector<std::vector<pcl::PointIndices>> clusters(3);
    ec.extractBatch(clouds, clusters);  // nothing to do
    CHECK(clusters.empty());
    auto cloud = boost::make_shared<pcl::PointCloud<P>>();
    cloud->push_back(P{});
    clouds.push_back(cloud);
    clouds.push_back(typename Ec::PointCloudConstPtr());
    clusters.resize(2);
    ec.extractBatch(clouds, clusters);  // a null cloud: refused
    CHECK(clusters.empty());
    clouds.pop_back();
    clouds.push_back(cloud);
    clusters.resize(2);
    ec.extractBatch(clouds, clusters);  // no device to open: logged, nothing
    CHECK(clusters.empty());
    CHECK(!ec.getInputCloud());
}

int main() {
    none<pcl::PointXYZ>();
    none<Point32>();
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
