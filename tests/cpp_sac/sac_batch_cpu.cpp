// segmentBatch links for pcl::PointXYZ (precompiled in libwave_matching.so) and for a 32-byte point type (through the
// impl header).  No device here: an empty queue and a queue without a cloud of three points return before one is
// needed, a null cloud is logged, and a queue that needs a device logs the failure and gives empty outputs.
#include <cstdio>
#include <vector>

#include "wave/matching/impl/sac_segmentation.hpp"
#include "wave/matching/sac_segmentation.hpp"

struct alignas(16) Point32 {
    float x, y, z, pad;
    float intensity, ring, a, b;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::SACSegmentation<Point32>;

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
    using Seg = wave::SACSegmentation<P>;
    Seg seg;
    seg.setDistanceThreshold(0.1);
    std::vector<typename Seg::PointCloudConstPtr> clouds;
    std::vector<pcl::PointIndices> idx(3);
    std::vector<pcl::ModelCoefficients> coef(3);
    seg.segmentBatch(clouds, idx, coef);  // nothing to do
    CHECK(idx.empty() && coef.empty());
    auto two = boost::make_shared<pcl::PointCloud<P>>();
    for (int i = 0; i < 2; ++i) {
        P p{};
        p.x = (float) i;
        two->push_back(p);
    }
    clouds.push_back(boost::make_shared<pcl::PointCloud<P>>());
    clouds.push_back(typename Seg::PointCloudConstPtr());
    clouds.push_back(two);
    seg.segmentBatch(clouds, idx, coef);  // no cloud with a sample, a null cloud: logged, empty outputs, no device
    CHECK(idx.size() == 3 && coef.size() == 3);
    for (const auto &i : idx) CHECK(i.indices.empty());
    for (const auto &c : coef) CHECK(c.values.empty());
    auto cloud = boost::make_shared<pcl::PointCloud<P>>();
    for (int i = 0; i < 5; ++i) {
        P p{};
        p.x = (float) i;
        p.y = (float) (i * i);
        cloud->push_back(p);
    }
    clouds.push_back(cloud);
    idx.clear();
    coef.clear();
    seg.segmentBatch(clouds, idx, coef);  // no device to open: logged, empty outputs
    CHECK(idx.size() == 4 && coef.size() == 4 && idx[3].indices.empty() && coef[3].values.empty());
}

int main() {
    none<pcl::PointXYZ>();
    none<Point32>();
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
